"""The doubly reparameterised gradient (include/gmvae_hip.h GMVAE_GRAD_DREG, csrc/kernels.hpp z_head_bwd_dreg) on the device,
through the C ABI: the step against the fp64 statement (tests/dreg_ref.py) at the gates of hip_util.compare_step, the bit's
effect on the inference gradient, everything generative unmoved against the standard step, the refusal and the routing,
train graphs against eager steps, and the Python surface."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import dreg_ref as DR
import oracle as O
from hip_util import _L, check_grads, dev, dims_of, hip_step, tail_gates

pytestmark = pytest.mark.gpu

LR = 1e-3
GATE = 1e-4
VAE_S3 = ("vae", O.Dims(D=96, L=5, K=1, hidden=(16,)), 5, 3, 0)
CASES = {       # name: (model, Dims, B, S, objective flags)
    "vae_s1": ("vae", O.Dims(D=96, L=5, K=1, hidden=(16,)), 5, 1, 0),                     # v = null, ragged L, B % 4 != 0
    "vae_s3": VAE_S3,                                                                     # v written by iwae_rows_terms
    "vae_l70_s65": ("vae", O.Dims(D=96, L=70, K=1, hidden=(16,)), 3, 65, 0),              # two lane passes over L, v by iwae_rows
    "vae_gmp_s3": ("vae_gmp", O.Dims(D=96, L=8, K=7, hidden=(16,)), 5, 3, 0),             # GMP prior form
    "vae_gmp_k80_s2": ("vae_gmp", O.Dims(D=96, L=4, K=80, hidden=(16,)), 2, 2, 0),        # large K
    "gmvae_marginal": ("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24)), 5, 1, 4),       # two hidden layers, S = 1
    "gmvae_marginal_iw_s1": ("gmvae", O.Dims(D=96, L=6, K=6, hidden=(16,)), 5, 1, 8),     # S = 1 routed to ymarg_rows
    "gmvae_marginal_iw_s3": ("gmvae", O.Dims(D=96, L=6, K=6, hidden=(16,)), 5, 3, 8),     # v from ymarg_iw_rows
    "gmvae_marginal_iw_s70": ("gmvae", O.Dims(D=96, L=6, K=6, hidden=(16,)), 2, 70, 8),   # large S
    "vae_s3_tanh": ("vae", O.Dims(D=96, L=5, K=1, hidden=(16,), act="tanh"), 5, 3, 0),
    "vae_s3_sigma_min": ("vae", O.Dims(D=96, L=5, K=1, hidden=(16,), sigma_min=0.97), 5, 3, 0),   # the clamp mask and the clamped sigma
}
MODELS = {"vae": O.MODEL_VAE, "vae_gmp": O.MODEL_VAE_GMP, "gmvae": O.MODEL_GMVAE}


def _rows_per_x(model, d, S):
    return S * d.K if model == O.MODEL_GMVAE else S


def _setup(model, d, B, S, seed=0):
    p = O.init_params(model, d, np.random.default_rng(seed))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.05, p[k].shape)
    flat = O.pack(model, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, model, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * _rows_per_x(model, d, S), d.L)).astype(np.float32)
    return flat, x, eps


def dstep(model, d, S, flat, x, eps, flags, seed=5, step=3, row0=0):
    """One gmvae_step at row0 with sched_flags = flags (eps None: in-kernel noise): dict(g [P] float64 gradient sums, tail [8], masks, dlogits [B, K] | None,
    schedule)."""
    L = _L()
    B = x.shape[0]
    u = None
    if eps is not None and model == O.MODEL_GMVAE and not flags & (L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW):
        u = np.random.default_rng(9).uniform(0.05, 0.95, (B * S, d.K))
    g, tail, masks, ws, cd = hip_step(model, dataclasses.replace(d, S=S), flat, x, eps, u, seed, step, want_masks=True, flags=flags,
                                      row0=row0, mask_rows=_rows_per_x(model, d, S), want_ws=True)
    dlogits = None
    if model == O.MODEL_GMVAE:
        off = L.workspace_offset(cd, model, "dlogits") // 4
        dlogits = ws[off:off + B * d.K].view(B, d.K).cpu().numpy().copy()
    return dict(g=g, tail=tail, masks=masks, dlogits=dlogits, schedule=L.step_schedule(cd, model))


def _tensors(model, d, gs):
    lay, _, _ = O.param_layout(model, d)
    return {name: gs[off:off + int(np.prod(shape))].reshape(shape) for name, shape, off in lay}


@pytest.fixture(scope="module")
def steps():
    """Per case: the inputs, the step with the bit and the standard step on the same inputs -- run once, shared, not modified."""
    cache = {}

    def get(name):
        if name not in cache:
            mname, d, B, S, obj = CASES[name]
            model = MODELS[mname]
            flat, x, eps = _setup(model, d, B, S, seed=len(name))
            cache[name] = dict(model=model, d=d, B=B, S=S, flat=flat, x=x, eps=eps,
                               dreg=dstep(model, d, S, flat, x, eps, obj | _L().GRAD_DREG),
                               std=dstep(model, d, S, flat, x, eps, obj))
        return cache[name]
    return get


# ------------------------------------------------------------------------------- 1. parity with the fp64 statement
def check_step(name, c, ref=None):
    """The gates of the step with the bit, c = dict(model, d, B, S, flat, x, eps, dreg = dstep's result); ref: the statement's
    (C, g) at those parameters where the caller has it already.  Returns the statement's C."""
    model, d, B, S = c["model"], c["d"], c["B"], c["S"]
    got = c["dreg"]
    assert got["schedule"].startswith("general") and got["schedule"].endswith("+dreg"), got["schedule"]
    p32 = O.unpack(model, d, c["flat"].astype(np.float64))
    Cc, g = ref or DR.loss_and_grads(model, d, p32, c["x"], c["eps"], S)
    tail_gates(name, got["tail"], B, Cc)
    # (the device's ReLU on the other side of a pre-activation that is zero to rounding: the statement takes its subgradient)
    check_grads(name, model, d, got["g"], g, B, got["masks"], Cc["pre"],
                lambda m: DR.loss_and_grads(model, d, p32, c["x"], c["eps"], S, relu_masks=m)[1], GATE)
    if got["dlogits"] is not None:
        ref = Cc["dlogits"] * B
        assert np.abs(got["dlogits"] - ref).max() <= GATE * max(np.abs(ref).max(), 1e-6)
    return Cc


@pytest.mark.parametrize("name", list(CASES))
def test_step_matches_fp64_statement(steps, name):
    c = steps(name)
    d = c["d"]
    Cc = check_step(name, c)
    if d.sigma_min > 0:               # the case is about the clamp: some units on it, some off it
        sig = Cc["sig_q"]
        assert (sig == d.sigma_min).any() and (sig > d.sigma_min).any()


# ------------------------------------------------------------------------------------ 2. the bit does something
def test_the_bit_changes_the_encoder_gradient(steps):
    c = steps("vae_s3")
    a, b = _tensors(c["model"], c["d"], c["dreg"]["g"]), _tensors(c["model"], c["d"], c["std"]["g"])
    worst = max(np.abs(a[k] - b[k]).max() / max(np.abs(b[k]).max(), 1e-6) for k in a if DR.is_inference(c["model"], k))
    assert worst > 10 * GATE, worst


# --------------------------------------------------------------------------------------- 3. what must not move
@pytest.mark.parametrize("name", list(CASES))
def test_generative_side_is_the_standard_step(steps, name):
    """S > 1: the tail, dlogits and every non-inference gradient tensor bit-identical to the standard step on the same inputs
    (both run the general schedule: the same launches up to z_head_bwd).  S = 1: at the parity gates (the standard step may take
    a fused schedule there)."""
    c = steps(name)
    model, d, S = c["model"], c["d"], c["S"]
    a, b = c["dreg"], c["std"]
    ta, tb = _tensors(model, d, a["g"]), _tensors(model, d, b["g"])
    rest = [k for k in ta if not DR.is_inference(model, k)]
    assert rest and len(rest) < len(ta)
    if S > 1:
        assert b["schedule"].startswith("general"), b["schedule"]
        assert np.array_equal(a["tail"], b["tail"])
        if a["dlogits"] is not None:
            assert np.array_equal(a["dlogits"], b["dlogits"])
        for k in rest:
            assert np.array_equal(ta[k], tb[k]), k
    else:
        np.testing.assert_allclose(a["tail"][:4], b["tail"][:4], rtol=GATE, atol=GATE)
        assert a["tail"][4] == b["tail"][4]
        if a["dlogits"] is not None:
            assert np.abs(a["dlogits"] - b["dlogits"]).max() <= GATE * max(np.abs(b["dlogits"]).max(), 1e-6)
        for k in rest:
            assert np.abs(ta[k] - tb[k]).max() <= GATE * max(np.abs(tb[k]).max(), 1e-6), k


# ------------------------------------------------------------------------------------- 4. refusal and routing
def test_gumbel_gmvae_is_refused_before_any_launch():
    import torch
    L = _L()
    d, B, S = O.Dims(D=96, L=6, K=6, hidden=(16,)), 5, 3
    flat, x, _ = _setup(O.MODEL_GMVAE, d, B, S)
    cd = dims_of(dataclasses.replace(d, S=S), B)
    P, _ = L.param_count(cd, O.MODEL_GMVAE)
    ws = torch.zeros(L.workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, dtype=torch.float32, device="cuda")
    cd.sched_flags = L.GRAD_DREG
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.lib.gmvae_step(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                          L.current_stream())
    torch.cuda.synchronize()
    assert rc == -2
    assert torch.isnan(grads).all()
    assert L.lib.gmvae_workspace_bytes(C.byref(cd), O.MODEL_GMVAE, C.byref(C.c_uint64())) == -2


def test_marginal_step_at_configs2_sizes_runs_the_general_schedule():
    L = _L()
    d, B = O.Dims(D=784, L=64, K=10, hidden=(64,)), 1024
    flat, x, _ = _setup(O.MODEL_GMVAE, d, B, 1, seed=2)
    r = dstep(O.MODEL_GMVAE, d, 1, flat, x, None, L.OBJ_MARGINAL_Y | L.GRAD_DREG)
    assert r["schedule"] == "general+marginal+dreg"
    assert np.isfinite(r["g"]).all() and np.isfinite(r["tail"]).all() and r["tail"][4] == B
    s = dstep(O.MODEL_GMVAE, d, 1, flat, x, None, L.OBJ_MARGINAL_Y)
    assert np.array_equal(r["tail"], s["tail"])                # (the same Philox rows, the same forward)
    ta, ts = _tensors(O.MODEL_GMVAE, d, r["g"]), _tensors(O.MODEL_GMVAE, d, s["g"])
    for k in ta:
        assert np.array_equal(ta[k], ts[k]) != DR.is_inference(O.MODEL_GMVAE, k), k


# ------------------------------------------------------------------------------------------------- 5. graphs
def _engine(model, d, seed, **kw):
    from gmvae_amd.engine import Engine
    return Engine(model, d.D, d.L, d.K, list(d.hidden), random_seed=seed, **kw)


@pytest.mark.parametrize("model,kw", [("gmvae", dict(y_inference="marginal_iw")), ("vae", dict())])
def test_train_graph_is_eager_steps_bit_for_bit(model, kw):
    import torch
    d, B, n = O.Dims(D=784, L=8, K=10 if model == "gmvae" else 1, hidden=(64,)), 16, 3
    xs = torch.from_numpy((np.random.default_rng(8).random((n, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a = _engine(model, d, 11, n_samples=3, grad_estimator="dreg", **kw)
    b = _engine(model, d, 11, n_samples=3, grad_estimator="dreg", **kw)
    s = _engine(model, d, 11, n_samples=3, **kw)
    for t in range(n):
        a.train_step(xs[t], lr=LR)
        s.train_step(xs[t], lr=LR)
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=n)
    sx.copy_(xs)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == n
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log[n - 1], a.grads[a.P:])
    assert not torch.equal(a.params.detach(), s.params.detach())      # (and it is not the standard estimator's trajectory)


# ----------------------------------------------------------------------------------------- 6. Python surface
def test_engine_steps_and_checkpoints():
    import torch
    from gmvae_amd import gmvae, vae
    d, B = O.Dims(D=784, L=8, K=10, hidden=(64,)), 16
    x = torch.from_numpy((np.random.default_rng(3).random((B, d.D)) < 0.87).astype(np.uint8)).cuda()
    made = ((lambda **kw: vae.create_vae(d.D, d.L, fcnet_hidden_sizes=[64], random_seed=2, n_samples=3, **kw)),
            (lambda **kw: vae.create_vae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=[64], random_seed=2, **kw)),
            (lambda **kw: gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=[64], random_seed=2, n_samples=3,
                                             y_inference="marginal_iw", **kw)),
            (lambda **kw: gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=[64], random_seed=2,
                                             y_inference="marginal", **kw)))
    for make in made:
        m, s = make(grad_estimator="dreg"), make()
        e = m._engine
        assert e.grad_estimator == "dreg" and s._engine.grad_estimator == "standard"
        assert e.dims(B).sched_flags & _L().GRAD_DREG and not s._engine.dims(B).sched_flags & _L().GRAD_DREG
        losses = [e.train_step(x, lr=LR)[0].item() / B for _ in range(3)]
        assert np.isfinite(losses).all() and e.global_step == 3
        assert list(m.state_dict()) == list(s.state_dict())
        s.load_state_dict(m.state_dict())
        assert torch.equal(s._engine.params.detach(), e.params.detach())
        s._engine.global_step = e.global_step                   # (the Philox key of the forward's noise)
        o = e.forward(x)                                        # forward-only passes ignore the estimator
        os_ = s._engine.forward(x)
        assert torch.equal(o["tail"], os_["tail"])


def test_runner_trains_with_the_flag(tmp_path):
    from gmvae_amd import run_gmvae
    m = run_gmvae.main(["--mode=train", "--model=gmvae", "--y_inference=marginal_iw", "--n_samples", "3", "--grad_estimator", "dreg",
                        "--batch_size=16", "--max_steps=11", "--summarise_every=4", f"--logdir={tmp_path}", "--random_seed=3",
                        "--synthetic_size=256"])
    e = m._engine
    assert e.grad_estimator == "dreg" and e.global_step >= 11
    import torch
    assert torch.isfinite(e.params).all() and np.isfinite(e.grads[e.P].item())
