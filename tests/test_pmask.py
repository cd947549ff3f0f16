"""The per-example observation mask (GMVAE_OBJ_PIXEL_MASK) on the device: the step through the C ABI on explicit noise against the
fp64 statement (tests/pmask_ref.py) at the project's gates -- loss and nll at 1e-4 relative, kl / nent as tests/test_wobj.py's
gates, every gradient tensor at 1e-4 of its own max, tail[5] at 1e-4 relative to itself, tail[6..7] exact, the dead rows and
columns exactly 0 -- then the flip invariance, the all-ones mask, gmvae_forward, gmvae_iw_bound, the graphs, the refusals and the
runner / model API.  x is flipped at the missing pixels in every case: any use of x there shows."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import oracle as O
import pmask_ref as PR
from hip_util import _L, check_grads, dev, dims_of, drop_comm, hip_step, need_rccl, tail_gates, write_inputs

pytestmark = pytest.mark.gpu

LR = 1e-3
SEED, STEP = 11, 3
_REF = {}          # case -> the fp64 statement's (C, g): computed once, shared, left unchanged


def _ref(name):
    if name not in _REF:
        model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
        _REF[name] = PR.loss_and_grads(model, d, p32, xf, eps, u, m)
    return _REF[name]


def _cdims(d, B, bit=True):
    cd = dims_of(d, B)
    cd.sched_flags = _L().OBJ_PIXEL_MASK if bit else 0
    return cd


def _fill_mask(ws, cd, model, mask):
    """mask (uint8 [B, D]) into slot 0 of the workspace's "pixel_mask" region."""
    write_inputs(ws, cd, model, {"pixel_mask": mask})


def pstep(model, d, flat, x, eps, u, mask, bit=True, row0=0):
    """One gmvae_step at row0 (slot 0 of the masks = mask): (grad sums [P] float64, tail [8], the step's ReLU masks)."""
    return hip_step(model, d, flat, x, eps, u, 5, 3, want_masks=True, flags=_L().OBJ_PIXEL_MASK if bit else 0, row0=row0,
                    inputs={"pixel_mask": mask} if bit else None)


def _dead_zeros(model, d, gs, what):
    """The dead columns (missing in every row): their rows of every encoder first-layer weight gradient and their columns of the
    decoder's output weight and bias gradients are exactly 0."""
    lay, _, _ = O.param_layout(model, d)
    dead = list(PR.dead_columns(d.D))
    nl = len(d.hidden)
    seen = 0
    for pname, shape, off in lay:
        g = gs[off:off + int(np.prod(shape))].reshape(shape)
        if pname in ("encoder_y_fcnet/linear_0/w", "encoder_gmm_fcnet/linear_0/w", "encoder_fcnet/linear_0/w"):
            assert (g[dead, :] == 0).all(), (what, pname)
            assert np.abs(g).max() > 0
            seen += 1
        elif pname == f"decoder_fcnet/linear_{nl}/w":
            assert (g[:, dead] == 0).all(), (what, pname)
            seen += 1
        elif pname == f"decoder_fcnet/linear_{nl}/b":
            assert (g.reshape(-1)[dead] == 0).all(), (what, pname)
            seen += 1
    assert seen >= 3


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.CASES))
def test_step_matches_fp64_statement(name):
    model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
    B = x.shape[0]
    L = _L()
    assert L.step_schedule(_cdims(d, B), model) == "general+mask"
    if name == "gumbel-784":
        assert L.step_schedule(_cdims(d, B, bit=False), model) != "general"
    gs, tail, masks = pstep(model, d, flat, xf, eps, u, m)
    Cc, g = _ref(name)
    tail_gates(name, tail, B, Cc)
    print(f"{name}: tail[5..7] {tail[5:].tolist()} ref hid {Cc['hid']} missing {Cc['n_missing']} observed {Cc['n_observed']}")
    assert abs(tail[5] - Cc["hid"]) <= 1e-4 * abs(Cc["hid"]), (tail[5], Cc["hid"])
    assert tail[6] == Cc["n_missing"] and tail[7] == Cc["n_observed"]
    if PR.CASES[name].lam_scale:
        lam = PR._decoder_logits(model, d, p32, x, eps, u, m)
        assert 50.0 <= np.abs(lam).max() <= 70.0
    check_grads(name, model, d, gs, g, B, masks, Cc["pre"],
                lambda mk: PR.loss_and_grads(model, d, p32, xf, eps, u, m, relu_masks=mk)[1])
    _dead_zeros(model, d, gs, name)


# 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "gumbel", "gmvae-s3", "gumbel-d99", "gumbel-784"])
def test_flip_invariance_bit_for_bit(name):
    """Gradients and tail[0..4] with x flipped at the missing pixels are the bits of the step with x zeroed there."""
    model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
    gf, tf, _ = pstep(model, d, flat, xf, eps, u, m)
    gz, tz, _ = pstep(model, d, flat, (x * (m != 0)).astype(np.uint8), eps, u, m)
    assert np.array_equal(gf, gz) and np.array_equal(tf[:5], tz[:5])
    assert np.array_equal(tf[6:], tz[6:]) and tf[5] != tz[5]


# 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "vae_gmp", "gumbel", "gmvae-s3", "gumbel-d99", "gumbel-784"])
def test_all_ones_mask_is_the_step_without_the_bit(name):
    model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
    B = x.shape[0]
    gw, tw, _ = pstep(model, d, flat, x, eps, u, np.full_like(m, 255))       # (any non-zero byte counts as observed)
    g0, t0, _ = pstep(model, d, flat, x, eps, u, None, bit=False)
    print(f"{name}: with the bit {tw.tolist()} without {t0.tolist()}")
    assert abs(tw[0] - t0[0]) <= 1e-4 * abs(t0[0]) and abs(tw[1] - t0[1]) <= 1e-4 * abs(t0[1])
    assert abs(tw[2] - t0[2]) <= 1e-4 * max(abs(t0[2]), B) and abs(tw[3] - t0[3]) <= 1e-4 * max(abs(t0[3]), B)
    assert tw[4] == t0[4] == B and tw[5] == 0 and tw[6] == 0 and tw[7] == B * d.D
    lay, _, _ = O.param_layout(model, d)
    for pname, shape, off in lay:
        n = int(np.prod(shape))
        err = np.abs(gw[off:off + n] - g0[off:off + n]).max() / max(np.abs(g0[off:off + n]).max(), 1e-6 * B)
        assert err <= 1e-4, (pname, err)


# 4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae_gmp", "gumbel", "gmvae-s3", "gumbel-784"])
def test_forward_row_terms(name):
    import torch
    L = _L()
    model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
    B, R = x.shape[0], x.shape[0] * d.S
    cd = _cdims(d, B)
    ws = torch.zeros(L.workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    _fill_mask(ws, cd, model, m)
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    rows = torch.full((R, 4), float("nan"), device="cuda")
    params, xd, ed = dev(flat, torch.float32), dev(xf, torch.uint8), dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    L.check(L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail), L.ptr(rows), None,
                                None, None, L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    Cc, _ = _ref(name)
    rows, tail = rows.cpu().numpy().astype(np.float64), tail.cpu().numpy().astype(np.float64)
    tail_gates(name, tail, B, Cc)
    assert abs(tail[5] - Cc["hid"]) <= 1e-4 * abs(Cc["hid"]) and tail[6] == Cc["n_missing"] and tail[7] == Cc["n_observed"]
    ref = Cc["rows"]
    for j, what in enumerate(("logpx", "logq", "logp", "logw")):
        gate = 1e-4 * np.maximum(np.abs(ref[:, j]), 1.0)
        assert (np.abs(rows[:, j] - ref[:, j]) <= gate).all(), (what, np.abs(rows[:, j] - ref[:, j]).max())
    assert (rows[:d.S, 0] == 0).all()                  # (row 0 observes nothing: its masked logpx is an empty sum)


# 5 --------------------------------------------------------------------------------------------------------------
def _iw(model, d, flat, x, mask, n, chunk):
    import torch
    L = _L()
    B = x.shape[0]
    cd = _cdims(dataclasses.replace(d, S=chunk), B)
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    _fill_mask(ws, cd, model, mask)
    bound, mlw = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, L.ptr(bound), L.ptr(mlw), L.ptr(tail), L.ptr(ws),
                                 SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    return bound.cpu().numpy(), mlw.cpu().numpy(), tail.cpu().numpy()


@pytest.mark.parametrize("name", ["vae_gmp", "gumbel", "gumbel-784"])
def test_iw_bound_on_the_observed_pixels(name):
    """n = 7 in chunks of 3 against the statement on the regenerated noise (Philox row (row0 + b) n + s); gumbel-784 has the
    sizes the one-launch evaluation would take without the bit."""
    n, chunk = 7, 3
    model, d, p32, flat, xf, eps, u, m, x = PR.setup(name)
    B = x.shape[0]
    ref = []
    for b in range(B):
        e, uu = O.noise(n, d.L, d.K, b * n, SEED, STEP)
        Cb, _ = PR.loss_and_grads(model, dataclasses.replace(d, S=n), p32, xf[b:b + 1], e, uu if model == O.MODEL_GMVAE else None,
                                  m[b:b + 1])
        ref.append(Cb["bound"][0])
    ref = np.array(ref)
    bound, mlw, tail = _iw(model, d, flat, xf, m, n, chunk)
    print(f"{name}: bound {bound.tolist()} ref {ref.tolist()}")
    assert np.all(np.abs(bound - ref) <= 1e-4 * np.maximum(np.abs(ref), 1.0)), (bound, ref)
    assert np.all(mlw <= bound + 1e-4 * np.abs(bound))
    assert tail[4] == B and (tail[5:] == 0).all() and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * abs(tail[0])
    one, _, _ = _iw(model, d, flat, xf, m, n, n)
    assert np.all(np.abs(one - bound) <= 1e-5 * np.maximum(np.abs(bound), 1.0))


# 6 --------------------------------------------------------------------------------------------------------------
def _engine(name, seed, **kw):
    from gmvae_amd.engine import Engine
    c = PR.CASES[name]
    d = c.d
    return Engine(c.mname, d.D, d.L, d.K, list(d.hidden), n_samples=d.S, random_seed=seed, temperature=d.temperature,
                  sigma_min=d.sigma_min, pixel_mask=True, **kw)


def _batches(d, B, n, seed):
    import torch
    rng = np.random.default_rng(seed)
    xs = torch.from_numpy((rng.random((n, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    ms = torch.from_numpy(np.stack([PR.make_mask(B, d.D, seed=seed + 1 + i) for i in range(n)])).cuda()
    return xs, ms


@pytest.mark.parametrize("name", ["gumbel", "vae-s3"])
def test_train_graph_reads_one_mask_per_step(name):
    """A three-step train graph with three different masks in slots 0-2 ends on the bits of three eager steps."""
    import torch
    d, B = PR.CASES[name].d, 16
    xs, ms = _batches(d, B, 3, 8)
    a, b = _engine(name, 11), _engine(name, 11)
    tails = [a.train_step(xs[t], lr=LR, mask=ms[t]).clone() for t in range(3)]
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=3)
    assert replay.pixel_mask.shape == (3, B, d.D) and bool((replay.pixel_mask == 1).all())      # pre-filled: all observed
    sx.copy_(xs)
    replay.pixel_mask.copy_(ms)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 3
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log, torch.stack(tails))
    assert len({t[6].item() for t in tails}) == 3      # (three different masks)
    with pytest.raises(ValueError):
        b.capture_train_step(B, lr=LR, n_steps=_L().LABEL_SLOTS + 1)
    with pytest.raises(ValueError, match="capture_train_step"):
        b.capture_train_pipeline(None, B, lr=LR, n_steps=2)


# 7 --------------------------------------------------------------------------------------------------------------
def test_dp_graph_with_a_one_rank_communicator():
    import torch
    need_rccl()
    L = _L()
    name = "gumbel"
    d, B = PR.CASES[name].d, 16
    xs, ms = _batches(d, B, 3, 10)
    a, b = _engine(name, 13), _engine(name, 13)
    b.enable_rccl()
    try:
        tails = [a.train_step(xs[t], lr=LR, mask=ms[t]).clone() for t in range(2)]
        sb, rb = b.capture_train_step(B, lr=LR, all_reduce=True, n_steps=2)
        assert b.dp_mode == "rccl-in-hipgraph"
        sb.copy_(xs[:2])
        rb.pixel_mask.copy_(ms[:2])
        rb()
        tails.append(a.train_step(xs[2], lr=LR, mask=ms[2]).clone())
        t3 = b.dp_step(xs[2], LR, mask=ms[2]).clone()
        torch.cuda.synchronize()
        for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
            assert torch.equal(u.detach(), v.detach())
        assert torch.equal(rb.tail_log, torch.stack(tails[:2])) and torch.equal(t3, tails[2])
    finally:
        drop_comm(b)


# 8 --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every refused combination returns GMVAE_E_DIMS and leaves the gradient buffer and the workspace as they were."""
    import torch
    L = _L()
    model, d, p32, flat, xf, eps, u, m, x = PR.setup("gumbel")
    B = x.shape[0]
    params, xd = dev(flat, torch.float32), dev(xf, torch.uint8)
    ok = _cdims(d, B)
    P, _ = L.param_count(ok, model)
    ws = torch.zeros(L.workspace_bytes(ok, model) // 4 + 64, dtype=torch.float32, device="cuda")
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    for extra in (L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.GRAD_DREG | L.OBJ_MARGINAL_Y, L.OBJ_LABELS | L.OBJ_MARGINAL_Y, L.OBJ_WEIGHTS,
                  L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH):
        cd = _cdims(d, B)
        cd.sched_flags |= extra
        assert L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 5, 3, None,
                                L.current_stream()) == -2
        assert L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(tail), None, None, None, None,
                                   L.ptr(ws), 0, 0, L.current_stream()) == -2
        assert L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), 4, None, None, L.ptr(tail), L.ptr(ws), 0, 0,
                                    L.current_stream()) == -2
    for fn in ("gmvae_iw_bound_enum_y", "gmvae_posterior_y"):
        args = (None, None) if fn == "gmvae_iw_bound_enum_y" else (None, None, None)
        assert getattr(L.lib, fn)(C.byref(ok), model, L.ptr(xd), L.ptr(params), 4, *args, L.ptr(tail), L.ptr(ws), 0, 0,
                                  L.current_stream()) == -2
    # the third refusing evaluator is the VAE_GMP's: real buffers of a vae_gmp case
    vmodel, vd, _, vflat, vxf, _, _, _, _ = PR.setup("vae_gmp")
    vparams, vxd = dev(vflat, torch.float32), dev(vxf, torch.uint8)
    vok = _cdims(vd, vxf.shape[0])
    vws = torch.zeros(L.workspace_bytes(vok, vmodel) // 4 + 64, dtype=torch.float32, device="cuda")
    assert L.lib.gmvae_posterior_component(C.byref(vok), vmodel, L.ptr(vxd), L.ptr(vparams), 4, None, None, None, L.ptr(tail),
                                           L.ptr(vws), 0, 0, L.current_stream()) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(grads).all()) and bool(torch.isnan(tail).all()) and bool((ws == 0).all()) and bool((vws == 0).all())
    from gmvae_amd.engine import Engine
    e = Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=1)
    with pytest.raises(ValueError, match="pixel_mask=True"):
        e.step(xd, mask=torch.from_numpy(m).cuda())
    pe = _engine("gumbel", 1)
    for call in (pe.iw_bound_enum_y, pe.posterior_y):
        with pytest.raises(ValueError, match="pixel_mask"):
            call(xd, 4)
    ve = Engine("vae_gmp", vd.D, vd.L, vd.K, list(vd.hidden), sigma_min=vd.sigma_min, random_seed=1, pixel_mask=True)
    with pytest.raises(ValueError, match="pixel_mask"):
        ve.posterior_component(vxd, 4)


# 9 --------------------------------------------------------------------------------------------------------------
def test_runner_trains_restores_and_evaluates_with_missing_pixels(tmp_path, capsys):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=32", "--max_steps=11", "--summarise_every=4", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=256", "--missing_rate=0.5", "--missing_seed=5"]
    model = run_gmvae.main(["--mode=train"] + args)
    assert runners.run_train.last_path == "graph+mask" and model._engine.pixel_mask and model._engine.global_step == 12
    res = run_gmvae.main(["--mode=eval", "--iw_samples=5"] + args)
    out = capsys.readouterr().out
    assert "train/imputation_nll" in out and "train/observed_share" in out and "train/loss_per_example" in out
    assert res["examples"] == 256 and abs(res["train/observed_share"] - 0.5) < 0.02
    assert 0.0 < res["train/imputation_nll"] < 2.0 and np.isfinite(res["train/iw_bound_5_per_example"])
    # the masked loss counts about half the pixels: far below the unmasked evaluation of the same checkpoint
    plain = run_gmvae.main(["--mode=eval"] + [a for a in args if not a.startswith("--missing")])
    assert res["train/loss_per_example"] < 0.7 * plain["train/loss_per_example"]
    # a checkpoint trained with masks loads in a model without them (above) and the other way round
    from gmvae_amd import gmvae
    kw = dict(mixture_components=10, fcnet_hidden_sizes=[64], sigma_min=0.0, raw_sigma_bias=0.5)
    m0 = gmvae.create_gmvae(784, 8, random_seed=9, **kw)
    m2 = gmvae.create_gmvae(784, 8, random_seed=7, pixel_mask=True, **kw)
    assert m0.state_dict().keys() == model.state_dict().keys()
    m2.load_state_dict(m0.state_dict())
    assert torch.equal(m2.params.detach(), m0.params.detach())
    # the model API: run_model with a mask, summaries, impute
    x = torch.from_numpy((np.random.default_rng(3).random((6, 784)) < 0.87).astype(np.uint8)).cuda()
    mk = torch.from_numpy(PR.make_mask(6, 784)).cuda()
    loss = m2.run_model(x, x, mask=mk)
    loss.backward()
    s = m2.summaries
    assert s["observed_share"].item() == pytest.approx(mk.float().mean().item(), rel=1e-6) and s["imputation_nll"].item() > 0
    assert torch.isfinite(m2.params.grad).all()
    m2.run_model(x, x)                                  # mask=None: all observed
    s = m2.summaries
    assert "imputation_nll" not in s and s["observed_share"].item() == 1.0
    imp = m2.impute(x, mk)
    assert imp.shape == x.shape and torch.equal(imp[mk != 0], x[mk != 0].to(imp.dtype))
    miss = imp[mk == 0]
    assert bool(((miss > 0) & (miss < 1)).all())
