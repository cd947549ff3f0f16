"""The likelihoods on grey-level bytes (GMVAE_LIK_*) on the device: the step through the C ABI on explicit noise against the fp64
statement (tests/lik_ref.py) at the project's gates, each term relative to the magnitude of its own addends (under these
likelihoods nll is a sum of mixed signs and can sit near 0) -- loss at 1e-4 of max(|loss|, nll_abs), nll at 1e-4 of nll_abs, kl /
nent at 1e-4 of max(|.|, 1), every gradient tensor at 1e-4 of its own max, tail[5] at 1e-4 relative to itself, tail[6..7] exact
-- then the tie to the Bernoulli step, gmvae_forward, gmvae_iw_bound, the graphs, sigma on the device, the refusals and the
model API / runner."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lik_ref as LR
import oracle as O
from hip_util import _L, check_grads, dev, dims_of, drop_comm, hip_step, need_rccl, write_inputs

pytestmark = pytest.mark.gpu

LR_ = 1e-3
SEED, STEP = 11, 3
_REF = {}          # case -> the fp64 statement's (C, g): computed once, shared, left unchanged


def _ref(name):
    if name not in _REF:
        model, d, p32, flat, x, eps, u = LR.setup(name)
        c = LR.CASES[name]
        _REF[name] = LR.loss_and_grads(model, d, p32, x, eps, u, c.lik, c.sigma)
    return _REF[name]


def _cdims(d, B, lik):
    cd = dims_of(d, B)
    cd.sched_flags = LR.FLAG[lik] if lik else 0
    return cd


def _inputs(lik, sigma):
    return {"lik_sigma": np.array([sigma], np.float32)} if lik == "gauss" else None


def lstep(model, d, flat, x, eps, u, lik, sigma=1.0, row0=0):
    """One gmvae_step at row0 under the likelihood (sigma in its workspace cell): (grad sums [P] float64, tail [8], the step's
    ReLU masks)."""
    return hip_step(model, d, flat, x, eps, u, 5, 3, want_masks=True, flags=LR.FLAG[lik] if lik else 0, row0=row0,
                    inputs=_inputs(lik, sigma))


def lik_gates(what, tail, B, Cc):
    """tail[0..4] against the statement's batch means, each term relative to the magnitude of its own addends."""
    print(f"{what}: tail {tail.tolist()} ref loss {Cc['loss']} nll {Cc['nll']} (abs {Cc['nll_abs']}) kl {Cc['kl']} nent {Cc['nent']}")
    print(f"{what}: err loss {abs(tail[0] / B - Cc['loss']):.3e} nll {abs(tail[1] / B - Cc['nll']):.3e} "
          f"kl {abs(tail[2] / B - Cc['kl']):.3e} nent {abs(tail[3] / B - Cc['nent']):.3e}")
    assert tail[4] == B
    assert abs(tail[0] / B - Cc["loss"]) <= 1e-4 * max(abs(Cc["loss"]), Cc["nll_abs"]), (what, tail[0] / B, Cc["loss"])
    assert abs(tail[1] / B - Cc["nll"]) <= 1e-4 * Cc["nll_abs"], (what, tail[1] / B, Cc["nll"])
    assert abs(tail[2] / B - Cc["kl"]) <= 1e-4 * max(abs(Cc["kl"]), 1.0), (what, tail[2] / B, Cc["kl"])
    assert abs(tail[3] / B - Cc["nent"]) <= 1e-4 * max(abs(Cc["nent"]), 1.0), (what, tail[3] / B, Cc["nent"])


def sq_gates(what, tail, B, D, Cc, zero=False):
    print(f"{what}: tail[5..7] {tail[5:].tolist()} ref sqerr {Cc['sqerr']}")
    if zero:
        assert abs(tail[5] - Cc["sqerr"]) <= 1e-6 * B * D, (what, tail[5], Cc["sqerr"])
    else:
        assert abs(tail[5] - Cc["sqerr"]) <= 1e-4 * abs(Cc["sqerr"]), (what, tail[5], Cc["sqerr"])
    assert tail[6] == B * D and tail[7] == 0


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LR.CASES))
def test_step_matches_fp64_statement(name):
    model, d, p32, flat, x, eps, u = LR.setup(name)
    c = LR.CASES[name]
    B = x.shape[0]
    L = _L()
    assert L.step_schedule(_cdims(d, B, c.lik), model) == "general" + LR.SUFFIX[c.lik]
    if name.startswith("gumbel-784"):
        assert L.step_schedule(_cdims(d, B, None), model) != "general"
    gs, tail, masks = lstep(model, d, flat, x, eps, u, c.lik, c.sigma)
    Cc, g = _ref(name)
    assert np.isfinite(gs).all() and np.isfinite(tail).all()
    lik_gates(name, tail, B, Cc)
    sq_gates(name, tail, B, d.D, Cc, zero=name == "vae-cb-zero")
    check_grads(name, model, d, gs, g, B, masks, Cc["pre"],
                lambda mk: LR.loss_and_grads(model, d, p32, x, eps, u, c.lik, c.sigma, relu_masks=mk)[1])
    if name == "vae-cb-zero":       # lambda == 0: logpx == 0, g = 1/2 - t -- the decoder-bias gradient is its column sum
        lay, _, _ = O.param_layout(model, d)
        off = {n: o for n, _, o in lay}[f"decoder_fcnet/linear_{len(d.hidden)}/b"]
        want = (0.5 - LR.targets(x)).sum(axis=0)
        assert np.abs(gs[off:off + d.D] - want).max() <= 1e-6 * np.abs(want).max()
        assert abs(tail[1]) <= 1e-6 * B * d.D


# 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae-grey", "gumbel-cb", "gumbel-784-grey"])
def test_grey_bernoulli_on_0_255_is_the_bernoulli_step(name):
    """grey_bernoulli on bytes in {0, 255} against the step without the field on the bytes in {0, 1}: at the gates, not bit for
    bit -- the first layers read fp32 t through another operand path."""
    model, d, p32, flat, x, eps, u = LR.setup(name)
    B = x.shape[0]
    x01 = (x >= 128).astype(np.uint8)
    gw, tw, _ = lstep(model, d, flat, (x01 * 255).astype(np.uint8), eps, u, "grey")
    g0, t0, _ = lstep(model, d, flat, x01, eps, u, None)
    print(f"{name}: with the field {tw.tolist()} without {t0.tolist()}")
    assert abs(tw[0] - t0[0]) <= 1e-4 * abs(t0[0]) and abs(tw[1] - t0[1]) <= 1e-4 * abs(t0[1])
    assert abs(tw[2] - t0[2]) <= 1e-4 * max(abs(t0[2]), B) and abs(tw[3] - t0[3]) <= 1e-4 * max(abs(t0[3]), B)
    assert tw[4] == t0[4] == B and tw[5] > 0 and tw[6] == B * d.D and tw[7] == 0
    lay, _, _ = O.param_layout(model, d)
    for pname, shape, off in lay:
        n = int(np.prod(shape))
        err = np.abs(gw[off:off + n] - g0[off:off + n]).max() / max(np.abs(g0[off:off + n]).max(), 1e-6 * B)
        assert err <= 1e-4, (pname, err)


# 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae_gmp-cb", "gmvae-s3-gauss", "gumbel-784-grey"])
def test_forward_row_terms(name):
    import torch
    L = _L()
    model, d, p32, flat, x, eps, u = LR.setup(name)
    c = LR.CASES[name]
    B, R = x.shape[0], x.shape[0] * d.S
    cd = _cdims(d, B, c.lik)
    ws = torch.zeros(L.workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    if c.lik == "gauss":
        write_inputs(ws, cd, model, _inputs(c.lik, c.sigma))
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    rows = torch.full((R, 4), float("nan"), device="cuda")
    params, xd, ed = dev(flat, torch.float32), dev(x, torch.uint8), dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    L.check(L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail), L.ptr(rows), None,
                                None, None, L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    Cc, _ = _ref(name)
    rows, tail = rows.cpu().numpy().astype(np.float64), tail.cpu().numpy().astype(np.float64)
    lik_gates(name, tail, B, Cc)
    sq_gates(name, tail, B, d.D, Cc)
    ref = Cc["rows"]
    mag = Cc["nll_abs"]        # (logpx and log w are sums of mixed signs: relative to the magnitude of their addends)
    for j, what in enumerate(("logpx", "logq", "logp", "logw")):
        gate = 1e-4 * np.maximum(np.abs(ref[:, j]), max(mag, 1.0) if j in (0, 3) else 1.0)
        assert (np.abs(rows[:, j] - ref[:, j]) <= gate).all(), (what, np.abs(rows[:, j] - ref[:, j]).max())


# 4 --------------------------------------------------------------------------------------------------------------
def _iw(model, d, flat, x, lik, sigma, n, chunk):
    import torch
    L = _L()
    B = x.shape[0]
    cd = _cdims(dataclasses.replace(d, S=chunk), B, lik)
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    if lik == "gauss":
        write_inputs(ws, cd, model, _inputs(lik, sigma))
    bound, mlw = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, L.ptr(bound), L.ptr(mlw), L.ptr(tail), L.ptr(ws),
                                 SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    return bound.cpu().numpy(), mlw.cpu().numpy(), tail.cpu().numpy()


@pytest.mark.parametrize("name", ["vae-grey", "gumbel-cb", "gmvae-s3-gauss"])
def test_iw_bound_under_the_likelihood(name):
    """n = 7 in chunks of 3 (n no multiple of the chunk) against the statement on the regenerated noise (Philox row
    (row0 + b) n + s)."""
    n, chunk = 7, 3
    model, d, p32, flat, x, eps, u = LR.setup(name)
    c = LR.CASES[name]
    B = x.shape[0]
    ref, mag = [], []
    for b in range(B):
        e, uu = O.noise(n, d.L, d.K, b * n, SEED, STEP)
        Cb, _ = LR.loss_and_grads(model, dataclasses.replace(d, S=n), p32, x[b:b + 1], e, uu if model == O.MODEL_GMVAE else None,
                                  c.lik, c.sigma)
        ref.append(Cb["bound"][0])
        mag.append(Cb["nll_abs"])
    ref, mag = np.array(ref), np.array(mag)
    bound, mlw, tail = _iw(model, d, flat, x, c.lik, c.sigma, n, chunk)
    print(f"{name}: bound {bound.tolist()} ref {ref.tolist()}")
    gate = 1e-4 * np.maximum(np.maximum(np.abs(ref), mag), 1.0)
    assert np.all(np.abs(bound - ref) <= gate), (bound, ref)
    assert np.all(mlw <= bound + gate)
    assert tail[4] == B and (tail[5:] == 0).all() and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * max(abs(tail[0]), mag.sum())
    one, _, _ = _iw(model, d, flat, x, c.lik, c.sigma, n, n)
    assert np.all(np.abs(one - bound) <= 0.1 * gate)


# 5 --------------------------------------------------------------------------------------------------------------
def _engine(gname, seed, **kw):
    from gmvae_amd.engine import Engine
    mname, d, lik, sigma = LR.GRAPH_CASES[gname]
    return Engine(mname, d.D, d.L, d.K, list(d.hidden), n_samples=d.S, random_seed=seed, temperature=d.temperature,
                  sigma_min=d.sigma_min, likelihood=LR.NAME[lik], likelihood_sigma=sigma, **kw)


def _batches(d, B, n, seed):
    import torch
    return torch.from_numpy(np.stack([LR.grey_batch(B, d.D, seed=seed + i) for i in range(n)])).cuda()


@pytest.mark.parametrize("gname,clip", [("gumbel-cb", None), ("vae-s3-gauss", None), ("vae-s3-gauss", 0.5)])
def test_train_graph_is_three_eager_steps(gname, clip):
    """A three-step train graph ends on the bits of three eager steps: parameters, m, v and the tails (with clip_norm too)."""
    import torch
    d, B = LR.GRAPH_CASES[gname][1], 16
    xs = _batches(d, B, 3, 8)
    kw = dict(clip_norm=clip) if clip else {}
    a, b = _engine(gname, 11, **kw), _engine(gname, 11, **kw)
    tails = [a.train_step(xs[t], lr=LR_).clone() for t in range(3)]
    sx, replay = b.capture_train_step(B, lr=LR_, n_steps=3)
    sx.copy_(xs)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 3
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log, torch.stack(tails))
    tl = replay.tail_log.cpu()
    assert bool(torch.isfinite(tl).all()) and bool((tl[:, 5] > 0).all()) and bool((tl[:, 6] == B * d.D).all()) and bool((tl[:, 7] == 0).all())
    assert not torch.equal(a.params.detach(), _engine(gname, 11, **kw).params.detach())      # (the steps moved the parameters)
    if clip:
        assert bool((replay.grad_clip[:, 0] > 0).all())
    with pytest.raises(ValueError, match="binarises"):
        b.capture_train_pipeline(None, B, lr=LR_, n_steps=2)


# 6 --------------------------------------------------------------------------------------------------------------
def test_dp_graph_with_a_one_rank_communicator():
    import torch
    need_rccl()
    gname = "gumbel-cb"
    d, B = LR.GRAPH_CASES[gname][1], 16
    xs = _batches(d, B, 3, 10)
    a, b = _engine(gname, 13), _engine(gname, 13)
    b.enable_rccl()
    try:
        tails = [a.train_step(xs[t], lr=LR_).clone() for t in range(2)]
        sb, rb = b.capture_train_step(B, lr=LR_, all_reduce=True, n_steps=2)
        assert b.dp_mode == "rccl-in-hipgraph"
        sb.copy_(xs[:2])
        rb()
        tails.append(a.train_step(xs[2], lr=LR_).clone())
        t3 = b.dp_step(xs[2], LR_).clone()
        torch.cuda.synchronize()
        for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
            assert torch.equal(u.detach(), v.detach())
        assert torch.equal(rb.tail_log, torch.stack(tails[:2])) and torch.equal(t3, tails[2])
    finally:
        drop_comm(b)


# 7 --------------------------------------------------------------------------------------------------------------
def test_sigma_is_read_from_device_memory():
    """The same captured Gaussian graph replayed after another sigma was written into "lik_sigma": the second replay matches the
    statement at the new sigma (on the parameters the first replay left, the step's own Philox noise)."""
    import torch
    gname = "vae-s3-gauss"
    mname, d, lik, sigma = LR.GRAPH_CASES[gname]
    model, B = O.MODEL_NAMES[mname], 8
    e = _engine(gname, 5)
    x = LR.grey_batch(B, d.D, seed=21)
    sx, replay = e.capture_train_step(B, lr=LR_, n_steps=1)
    sx.copy_(torch.from_numpy(x).cuda().view(sx.shape))
    for step, s in ((0, sigma), (1, 0.6)):
        e.set_likelihood_sigma(s)
        flat = e.params.detach().cpu().numpy().astype(np.float64)
        replay()
        torch.cuda.synchronize()
        tail = replay.tail_log.cpu().numpy().astype(np.float64).reshape(-1)
        eps, u = O.noise(B * d.S, d.L, d.K, 0, e.noise_seed, step)
        Cc, _ = LR.loss_and_grads(model, d, O.unpack(model, d, flat), x, eps, None, lik, s)
        lik_gates(f"{gname} sigma {s}", tail, B, Cc)
        sq_gates(f"{gname} sigma {s}", tail, B, d.D, Cc)
        if step == 1:      # (the gates tell the two sigmas apart: the statement at the old sigma is far outside them)
            Co, _ = LR.loss_and_grads(model, d, O.unpack(model, d, flat), x, eps, None, lik, sigma)
            assert abs(Co["nll"] - Cc["nll"]) >= 100 * 1e-4 * Cc["nll_abs"]
    assert e.global_step == 2


# 8 --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every refused combination returns GMVAE_E_DIMS and leaves the gradient buffer and the workspace as they were."""
    import torch
    L = _L()
    model, d, p32, flat, x, eps, u = LR.setup("gumbel-cb")
    B = x.shape[0]
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    ok = _cdims(d, B, "cb")
    P, _ = L.param_count(ok, model)
    ws = torch.zeros(L.workspace_bytes(ok, model) // 4 + 64, dtype=torch.float32, device="cuda")
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    for lik in LR.LIKS:
        for extra in (L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.GRAD_DREG | L.OBJ_MARGINAL_Y, L.OBJ_LABELS | L.OBJ_MARGINAL_Y, L.OBJ_WEIGHTS,
                      L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH, L.OBJ_PIXEL_MASK):
            cd = _cdims(d, B, lik)
            cd.sched_flags |= extra
            assert L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 5, 3, None,
                                    L.current_stream()) == -2
            assert L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(tail), None, None, None, None,
                                       L.ptr(ws), 0, 0, L.current_stream()) == -2
            assert L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), 4, None, None, L.ptr(tail), L.ptr(ws), 0, 0,
                                        L.current_stream()) == -2
        okl = _cdims(d, B, lik)
        for fn in ("gmvae_iw_bound_enum_y", "gmvae_posterior_y"):
            args = (None, None) if fn == "gmvae_iw_bound_enum_y" else (None, None, None)
            assert getattr(L.lib, fn)(C.byref(okl), model, L.ptr(xd), L.ptr(params), 4, *args, L.ptr(tail), L.ptr(ws), 0, 0,
                                      L.current_stream()) == -2
    # the third refusing evaluator is the VAE_GMP's: real buffers of a vae_gmp case
    vmodel, vd, _, vflat, vx, _, _ = LR.setup("vae_gmp-cb")
    vparams, vxd = dev(vflat, torch.float32), dev(vx, torch.uint8)
    vok = _cdims(vd, vx.shape[0], "cb")
    vws = torch.zeros(L.workspace_bytes(vok, vmodel) // 4 + 64, dtype=torch.float32, device="cuda")
    assert L.lib.gmvae_posterior_component(C.byref(vok), vmodel, L.ptr(vxd), L.ptr(vparams), 4, None, None, None, L.ptr(tail),
                                           L.ptr(vws), 0, 0, L.current_stream()) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(grads).all()) and bool(torch.isnan(tail).all()) and bool((ws == 0).all()) and bool((vws == 0).all())
    from gmvae_amd.engine import Engine
    pe = Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=1, likelihood="continuous_bernoulli")
    for call in (pe.iw_bound_enum_y, pe.posterior_y):
        with pytest.raises(ValueError, match="likelihood"):
            call(xd, 4)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        pe.step(torch.full((B, d.D), 1.5, device="cuda"))
    with pytest.raises(ValueError, match="gaussian"):
        pe.set_likelihood_sigma(0.5)
    ve = Engine("vae_gmp", vd.D, vd.L, vd.K, list(vd.hidden), sigma_min=vd.sigma_min, random_seed=1, likelihood="gaussian")
    with pytest.raises(ValueError, match="likelihood"):
        ve.posterior_component(vxd, 4)
    with pytest.raises(ValueError, match="likelihood_sigma"):
        ve.set_likelihood_sigma(0.0)


# 9 --------------------------------------------------------------------------------------------------------------
def test_model_api():
    import torch
    from gmvae_amd import gmvae
    d = O.Dims(D=100, L=5, K=7, hidden=(24,), sigma_min=0.001, raw_sigma_bias=0.25)
    model, B = O.MODEL_GMVAE, 8
    m = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=4,
                           likelihood="continuous_bernoulli")
    e = m._engine
    x = LR.grey_batch(B, d.D, seed=31)
    _, eps, u = O.make_inputs(d, B, model)
    xt = torch.from_numpy(x).cuda()
    loss = m.run_model(xt, xt, eps=torch.from_numpy(eps).cuda(), u=torch.from_numpy(u).cuda())
    p32 = O.unpack(model, d, e.params.detach().cpu().numpy().astype(np.float64))
    Cc, _ = LR.loss_and_grads(model, d, p32, x, eps, u, "cb")
    assert abs(loss.item() - Cc["loss"]) <= 1e-4 * max(abs(Cc["loss"]), Cc["nll_abs"]), (loss.item(), Cc["loss"])
    s = m.summaries
    assert abs(s["recon_mse"].item() - Cc["sqerr"] / (B * d.D)) <= 1e-4 * Cc["sqerr"] / (B * d.D)
    # a float image in [0, 1] is rounded to the nearest k / 255: the same step
    xf = xt.float() / 255.0
    loss_f = m.run_model(xf, xf, eps=torch.from_numpy(eps).cuda(), u=torch.from_numpy(u).cuda())
    assert loss_f.item() == loss.item()
    # decoder(z).mean() is A'(lambda)
    z = torch.randn(6, d.L, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 3.0
    dist = m.decoder(z)
    assert type(dist).__name__ == "ContinuousBernoulli"
    lam = dist.logits.double().cpu()
    assert (dist.mean().double().cpu() - LR.cb_mean(lam)).abs().max() <= 1e-5
    rec = m.reconstruct_images(xt)
    assert rec.shape == (B, d.D) and bool(((rec >= 0) & (rec <= 1)).all()) and bool(torch.isfinite(rec).all())
    gen = m.generate_sample_images(num_samples=2)
    assert bool(((gen >= 0) & (gen <= 1)).all())
    # the Gaussian's decoder returns its mean lambda itself
    g = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=4,
                           likelihood="gaussian", likelihood_sigma=0.25)
    dg = g.decoder(z)
    assert type(dg).__name__ == "NormalFixedScale" and dg.sigma == 0.25 and torch.equal(dg.mean(), dg.loc)
    assert torch.equal(g.params.detach(), m.params.detach())       # (the same parameters under every likelihood)


# 10 -------------------------------------------------------------------------------------------------------------
def test_runner_trains_restores_and_evaluates_on_grey_levels(tmp_path, capsys):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=32", "--max_steps=11", "--summarise_every=4", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=256", "--likelihood=gaussian", "--likelihood_sigma=0.25"]
    model = run_gmvae.main(["--mode=train"] + args)
    e = model._engine
    assert runners.run_train.last_path == "graph+grey" and e.likelihood == "gaussian" and e.likelihood_sigma == 0.25 and e.global_step == 12
    out = capsys.readouterr().out
    assert "recon_mse" in out and "loss:" in out
    sd = torch.load(runners._ckpt(run_gmvae.build_parser().parse_args(args)), map_location="cpu")
    assert sd["likelihood"] == "gaussian" and float(sd["likelihood_sigma"]) == 0.25
    # a second run restores the checkpoint bit for bit (and has no step left to take)
    again = run_gmvae.main(["--mode=train"] + args)
    assert "restored" in capsys.readouterr().out and again._engine.global_step == 12
    for u, v in ((model.params, again.params), (e.m, again._engine.m), (e.v, again._engine.v)):
        assert torch.equal(u.detach(), v.detach())
    res = run_gmvae.main(["--mode=eval", "--iw_samples=5"] + args)
    out = capsys.readouterr().out
    assert "train/recon_mse" in out and "train/loss_per_example" in out
    assert res["examples"] == 256 and 0.0 < res["train/recon_mse"] < 0.5 and np.isfinite(res["train/loss_per_example"])
    assert np.isfinite(res["train/iw_bound_5_per_example"])
    # restoring under another likelihood (or another sigma) is an error
    other = [a for a in args if not a.startswith("--likelihood")]
    for extra in (["--likelihood=continuous_bernoulli"], [], ["--likelihood=gaussian", "--likelihood_sigma=0.5"]):
        with pytest.raises(ValueError, match="cannot be restored"):
            run_gmvae.main(["--mode=eval"] + other + extra)
