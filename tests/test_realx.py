"""Real-valued data and the learned Gaussian scale (GMVAE_X_F32, GMVAE_LIK_SCALE_LEARNED) on the device: the step through the C
ABI on explicit noise against the fp64 statement (tests/realx_ref.py) at the gates of tests/test_lik.py -- the loss at 1e-4 of
max(|loss|, nll_abs), nll at 1e-4 of nll_abs, kl / nent at 1e-4 of max(|.|, 1), every gradient tensor (rho's included) at 1e-4 of
its own max, tail[5] at 1e-4 relative to itself, tail[6..7] exact --, then the bit-for-bit identities (the fp32 step on
bytes / 255 is the grey Gaussian step; a train graph is its eager steps; the one-rank data-parallel graph is the eager dp_step),
rho under TF-Adam, gmvae_iw_bound, gmvae_forward, the refusals, the model API and the runner.

Measured on an MI355X (profiles/realx_notes.md has the table): every case of test_step_matches_fp64_statement sits inside the
standing gates (worst: loss 1.4e-7, kl 7.3e-6, gradients 8.3e-6, rho 2.7e-7 of their gates' scales); of gmvae_forward's per-row
terms one case, gmvae-784-learned, misses log q for its conditioning alone and takes the measured allowance (CONDITIONED)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import adam_ref as AR
import lik_ref as LR
import oracle as O
import realx_ref as RR
from hip_util import _L, check_grads, dev, device_masks, dims_of, drop_comm, need_rccl, workspace, write_inputs
from test_lik import lik_gates, sq_gates

pytestmark = pytest.mark.gpu

LR_ = 1e-3
SEED, STEP = 11, 3
_REF = {}          # (case, scale) -> the fp64 statement's (C, g): computed once, shared, left unchanged


def _ref(name, scale):
    if (name, scale) not in _REF:
        model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, scale)
        _REF[(name, scale)] = RR.loss_and_grads(model, d, p32, t, eps, u, sigma=RR.CASES[name].sigma, rho=rho)
    return _REF[(name, scale)]


def _cdims(d, B, fl):
    cd = dims_of(d, B)
    cd.sched_flags = fl
    return cd


def _xdev(x):
    import torch
    return dev(x, torch.uint8 if x.dtype == np.uint8 else torch.float32)


def _ws(cd, model, sigma):
    """The step's workspace, zeroed, sigma in its cell where the dims have one (the fixed scale)."""
    ws = workspace(cd, model)
    if not cd.sched_flags & RR.LIK_SCALE_LEARNED:
        write_inputs(ws, cd, model, {"lik_sigma": np.array([sigma], np.float32)})
    return ws


def rstep(model, d, flat, x, eps, u, fl, sigma, seed=5, step=3, stale_rho_slabs=False, row0=0):
    """One gmvae_step at row0 under the flags (x uint8 or float32 as given): (grad sums [P] float64, tail [8], the step's ReLU masks).
    stale_rho_slabs: rho's range of every split-K slab of the gradient behind the first holds NaN when the step starts."""
    import torch
    L = _L()
    B = x.shape[0]
    cd = _cdims(d, B, fl)
    cd.row0 = row0
    P, _ = L.param_count(cd, model)
    assert P == flat.shape[0]
    params, xd = dev(flat, torch.float32), _xdev(x)
    ed = None if eps is None else dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    ws = _ws(cd, model, sigma)
    if stale_rho_slabs:
        D4, NS = RR.pad4(d.D), min(max(B * d.S // 256, 1), 16)          # (gmvae_hip.hip num_splits(R): the slabs a step sums)
        assert fl & RR.LIK_SCALE_LEARNED and NS > 1
        off = C.c_uint64()
        L.check(L.lib.gmvae_workspace_offset(C.byref(cd), model, b"slabs", C.byref(off)), "offset slabs")
        for k in range(1, NS):
            at = off.value // 4 + k * P + (P - D4)
            ws[at:at + D4] = float("nan")
    L.check(L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws), seed, step,
                             None, L.current_stream()), "gmvae_step")
    torch.cuda.synchronize()
    g = grads.cpu().numpy().astype(np.float64)
    return g[:P], g[P:], device_masks(ws, cd, model, d, B), grads.cpu()


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", RR.VARIANTS)
def test_step_matches_fp64_statement(name, scale):
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, scale)
    c = RR.CASES[name]
    B, D = x.shape[0], d.D
    L = _L()
    fl = RR.flags(c, scale)
    assert L.step_schedule(_cdims(d, B, fl), model) == "general" + RR.suffix(c, scale)
    gs, tail, masks, _ = rstep(model, d, flat, x, eps, u, fl, c.sigma)
    Cc, g = _ref(name, scale)
    what = f"{name}-{scale}"
    assert np.isfinite(gs).all() and np.isfinite(tail).all()
    lik_gates(what, tail, B, Cc)
    sq_gates(what, tail, B, D, Cc)
    check_grads(what, model, d, gs, g, B, masks, Cc["pre"],
                lambda mk: RR.loss_and_grads(model, d, p32, t, eps, u, sigma=c.sigma, rho=rho, relu_masks=mk)[1])
    if scale == "learned":
        P0 = flat.shape[0] - RR.pad4(D)
        got, ref = gs[P0:P0 + D] / B, g[RR.LOG_SIGMA]
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
        print(f"{what} {RR.LOG_SIGMA}: rel-to-max err {err:.3e}")
        assert err <= 1e-4, (what, err)
        assert not gs[P0 + D:].any()                                # (the pad behind rho's D values)


@pytest.mark.parametrize("name", ["gmvae-r650", "vae-r16450"])
def test_rho_range_of_every_slab_is_rewritten(name):
    """NS = 2 and 16 split-K slabs: liksig_finish owns rho's range in ALL of them (its sum to slab 0, zeros to the others).  A step
    that starts with NaN there -- what an earlier step of other sizes may have left -- ends on the bits of the step in a zeroed
    workspace."""
    import torch
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, "learned")
    c = RR.CASES[name]
    fl = RR.flags(c, "learned")
    _, _, _, clean = rstep(model, d, flat, x, eps, u, fl, c.sigma)
    _, _, _, stale = rstep(model, d, flat, x, eps, u, fl, c.sigma, stale_rho_slabs=True)
    assert bool(torch.isfinite(clean).all()) and torch.equal(clean, stale)


# 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lname", ["gmvae-s3-gauss", "gumbel-d99-gauss", "gumbel-784-gauss", "vae-gauss-sigma-small"])
def test_f32_step_on_bytes_over_255_is_the_grey_gaussian_step(lname):
    """The fp32 step on np.float32(b) / np.float32(255) with the fixed sigma against the grey-level Gaussian step on the bytes b:
    the same gradient buffer and tail, bit for bit (the division is correctly rounded on both sides: the same t)."""
    import torch
    model, d, p32, flat, xb, eps, u = LR.setup(lname)
    s = LR.CASES[lname].sigma
    xf = xb.astype(np.float32) / np.float32(255)
    assert xf.dtype == np.float32
    _, tb, _, gb = rstep(model, d, flat, xb, eps, u, RR.LIK_GAUSSIAN, s)
    _, tf, _, gf = rstep(model, d, flat, xf, eps, u, RR.LIK_GAUSSIAN | RR.X_F32, s)
    assert bool(torch.isfinite(gb).all()) and tb[5] > 0
    assert torch.equal(gb, gf), (lname, (gb - gf).abs().max().item(), tb.tolist(), tf.tolist())


# 3 --------------------------------------------------------------------------------------------------------------
ENGINES = {"gmvae": ("gmvae", RR.CASES["gmvae-2h"].d), "vae-s3": ("vae", O.Dims(D=96, L=4, K=1, hidden=(16,), S=3))}


def _engine(gname, seed, scale="learned", real=True, **kw):
    from gmvae_amd.engine import Engine
    mname, d = ENGINES[gname]
    return Engine(mname, d.D, d.L, d.K, list(d.hidden), n_samples=d.S, random_seed=seed, temperature=d.temperature,
                  sigma_min=d.sigma_min, likelihood="gaussian", likelihood_sigma=0.5, real_valued=real, likelihood_scale=scale, **kw)


def _batches(d, B, n, seed):
    import torch
    return torch.from_numpy(np.stack([RR.real_batch(B, d.D, seed=seed + i)[0] for i in range(n)])).cuda()


@pytest.mark.parametrize("gname,scale,clip", [("gmvae", "learned", None), ("vae-s3", "learned", 0.5), ("vae-s3", "fixed", None)])
def test_train_graph_is_three_eager_steps(gname, scale, clip):
    """A three-step train graph on float batches ends on the bits of three eager steps: parameters (rho among them), m, v and
    the tails -- with clip_norm too."""
    import torch
    d, B = ENGINES[gname][1], 16
    xs = _batches(d, B, 3, 8)
    kw = dict(clip_norm=clip) if clip else {}
    a, b = _engine(gname, 11, scale, **kw), _engine(gname, 11, scale, **kw)
    tails = [a.train_step(xs[t], lr=LR_).clone() for t in range(3)]
    sx, replay = b.capture_train_step(B, lr=LR_, n_steps=3)
    assert sx.dtype == torch.float32
    sx.copy_(xs)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 3
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log, torch.stack(tails))
    tl = replay.tail_log.cpu()
    assert bool(torch.isfinite(tl).all()) and bool((tl[:, 5] > 0).all()) and bool((tl[:, 6] == B * d.D).all()) and bool((tl[:, 7] == 0).all())
    fresh = _engine(gname, 11, scale, **kw)
    assert not torch.equal(a.params.detach(), fresh.params.detach())
    if scale == "learned":      # rho moved off ln(likelihood_sigma)
        rho0, rho = fresh.views()["decoder/log_sigma"], a.views()["decoder/log_sigma"]
        assert bool((rho0 == np.float32(np.log(0.5))).all()) and bool((rho != rho0).all())
    if clip:
        assert bool((replay.grad_clip[:, 0] > 0).all())


# 4 --------------------------------------------------------------------------------------------------------------
def test_dp_graph_with_a_one_rank_communicator():
    import torch
    need_rccl()
    d, B = ENGINES["gmvae"][1], 16
    xs = _batches(d, B, 3, 10)
    a, b = _engine("gmvae", 13), _engine("gmvae", 13)
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


# 5 --------------------------------------------------------------------------------------------------------------
def test_rho_under_tf_adam():
    """rho after each of three eager TF-Adam steps against the update statement (tests/adam_ref.py), element by element."""
    import torch
    d, B = ENGINES["vae-s3"][1], 16
    xs = _batches(d, B, 3, 20)
    e = _engine("vae-s3", 7)
    off = {n: o for n, _, o in e.layout}["decoder/log_sigma"]
    sl = slice(off, off + d.D)
    hp = AR.HP[1]
    for i in range(3):
        p0, m0, v0 = (t.detach()[sl].cpu().numpy() for t in (e.params, e.m, e.v))
        e.train_step(xs[i], lr=hp[0])
        torch.cuda.synchronize()
        gsum, count = e.grads[sl].cpu().numpy(), e.grads[e.P + 4].item()
        assert count == B and np.abs(gsum).max() > 0
        want = AR.predict(p0, m0, v0, gsum, count, i + 1, *hp)
        dm, dv, dp = AR.bounds(p0, m0, v0, gsum, count, i + 1, *hp)
        for what, got, ref, bound in (("rho", e.params.detach()[sl], want[0], dp), ("m", e.m[sl], want[1], dm), ("v", e.v[sl], want[2], dv)):
            r, j = AR.worst(got.cpu().numpy(), ref, bound)
            print(f"step {i + 1} {what}: worst error / bound {r:.3f} at {j}")
            assert r <= 1.0, (i, what, r, j)


# 6 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "gmvae-s3"])
def test_iw_bound_under_both_bits(name):
    """n = 7 in chunks of 3 against the statement on the regenerated noise (Philox row (row0 + b) n + s), x float, rho learned."""
    import torch
    L = _L()
    n, chunk = 7, 3
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, "learned")
    c = RR.CASES[name]
    B = x.shape[0]
    ref, mag = [], []
    for b in range(B):
        e, uu = O.noise(n, d.L, d.K, b * n, SEED, STEP)
        Cb, _ = RR.loss_and_grads(model, dataclasses.replace(d, S=n), p32, t[b:b + 1], e, uu if model == O.MODEL_GMVAE else None, rho=rho)
        ref.append(Cb["bound"][0])
        mag.append(Cb["nll_abs"])
    ref, mag = np.array(ref), np.array(mag)
    cd = _cdims(dataclasses.replace(d, S=chunk), B, RR.flags(c, "learned"))
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    bound, mlw = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    params, xd = dev(flat, torch.float32), _xdev(x)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, L.ptr(bound), L.ptr(mlw), L.ptr(tail), L.ptr(ws),
                                 SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    bound, mlw, tail = bound.cpu().numpy(), mlw.cpu().numpy(), tail.cpu().numpy()
    print(f"{name}: bound {bound.tolist()} ref {ref.tolist()}")
    gate = 1e-4 * np.maximum(np.maximum(np.abs(ref), mag), 1.0)
    assert np.all(np.abs(bound - ref) <= gate), (bound, ref)
    assert np.all(mlw <= bound + gate)
    assert tail[4] == B and (tail[5:] == 0).all()


# 7 --------------------------------------------------------------------------------------------------------------
# The cases whose per-row terms miss the standing gate for their conditioning alone: the x30 columns drive encoder_gmm's raw
# scale below -87, where sigma_q = softplus(.) is a denormal fp32 number and ln sigma_q keeps a few bits -- in ANY fp32
# evaluation.  Their allowance is measured, not chosen: 4x the error of the same statement in torch fp32 on the CPU against
# fp64 (realx_ref.terms_in), or the standing gate, whichever is larger.  Measured (profiles/realx_notes.md): gmvae-784-learned
# log q: device 1.69, torch fp32 6.37 (of |log q| up to 307; the standing gate there is 0.03).
CONDITIONED = {("gmvae-784", "learned")}


@pytest.mark.parametrize("name,scale", [("vae_gmp-tanh", "fixed"), ("gmvae-s3", "learned"), ("gmvae-784", "learned")])
def test_forward_row_terms(name, scale):
    """gmvae_forward's row terms (log p(x|z), log q, log p, log w per row) against the statement."""
    import torch
    L = _L()
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, scale)
    c = RR.CASES[name]
    B, R = x.shape[0], x.shape[0] * d.S
    cd = _cdims(d, B, RR.flags(c, scale))
    ws = _ws(cd, model, c.sigma)
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    rows = torch.full((R, 4), float("nan"), device="cuda")
    params, xd, ed = dev(flat, torch.float32), _xdev(x), dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    L.check(L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail), L.ptr(rows), None,
                                None, None, L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    Cc, _ = _ref(name, scale)
    rows, tail = rows.cpu().numpy().astype(np.float64), tail.cpu().numpy().astype(np.float64)
    lik_gates(name, tail, B, Cc)
    sq_gates(name, tail, B, d.D, Cc)
    ref, mag = Cc["rows"], Cc["nll_abs"]
    t32 = RR.terms_in(torch.float32, model, d, p32, t, eps, u, sigma=c.sigma, rho=rho)["rows"]
    for j, what in enumerate(("logpx", "logq", "logp", "logw")):
        gate = 1e-4 * np.maximum(np.abs(ref[:, j]), max(mag, 1.0) if j in (0, 3) else 1.0)
        e32 = np.abs(t32[:, j] - ref[:, j]).max()
        err = np.abs(rows[:, j] - ref[:, j])
        print(f"{name}-{scale} {what}: device err max {err.max():.3e} (worst err / standing gate {(err / gate).max():.3f}); "
              f"torch fp32 on the CPU err max {e32:.3e}")
        if (name, scale) in CONDITIONED:
            gate = np.maximum(gate, 4.0 * e32)
        assert (err <= gate).all(), (what, err.max())


# 8 --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every refused combination returns GMVAE_E_DIMS (an unaligned float x GMVAE_E_ALIGN) and leaves the gradient buffer and
    the workspace as they were."""
    import torch
    L = _L()
    model, d, p32, flat, x, t, eps, u, rho = RR.setup("gmvae-2h", "learned")
    B = x.shape[0]
    G, F, SL = RR.LIK_GAUSSIAN, RR.X_F32, RR.LIK_SCALE_LEARNED
    pad = torch.zeros(B * d.D + 4, dtype=torch.float32, device="cuda")
    pad[:B * d.D].copy_(torch.from_numpy(x).reshape(-1))
    params, xd = dev(flat, torch.float32), pad[:B * d.D]
    ok = _cdims(d, B, G | F | SL)
    P, _ = L.param_count(ok, model)
    ws = torch.zeros(L.iw_bound_workspace_bytes(ok, model) // 4 + 64, dtype=torch.float32, device="cuda")
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")

    def calls(cd, xp, want):
        assert L.lib.gmvae_step(C.byref(cd), model, xp, None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 5, 3, None,
                                L.current_stream()) == want
        assert L.lib.gmvae_forward(C.byref(cd), model, xp, None, None, L.ptr(params), L.ptr(tail), None, None, None, None,
                                   L.ptr(ws), 0, 0, L.current_stream()) == want
        assert L.lib.gmvae_iw_bound(C.byref(cd), model, xp, L.ptr(params), 4, None, None, L.ptr(tail), L.ptr(ws), 0, 0,
                                    L.current_stream()) == want

    for fl in (F, SL, F | SL, F | L.LIK_CONT_BERNOULLI, SL | L.LIK_GREY_BERNOULLI):
        calls(_cdims(d, B, fl), L.ptr(xd), -2)
    for extra in (L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.GRAD_DREG | L.OBJ_MARGINAL_Y, L.OBJ_LABELS | L.OBJ_MARGINAL_Y, L.OBJ_WEIGHTS,
                  L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH, L.OBJ_PIXEL_MASK):
        calls(_cdims(d, B, G | F | SL | extra), L.ptr(xd), -2)
    for fn in ("gmvae_iw_bound_enum_y", "gmvae_posterior_y"):
        args = (None, None) if fn == "gmvae_iw_bound_enum_y" else (None, None, None)
        assert getattr(L.lib, fn)(C.byref(ok), model, L.ptr(xd), L.ptr(params), 4, *args, L.ptr(tail), L.ptr(ws), 0, 0,
                                  L.current_stream()) == -2
    calls(ok, L.ptr(pad[1:B * d.D + 1]), -4)                         # a float x 4 bytes off a 16-byte boundary
    torch.cuda.synchronize()
    assert bool(torch.isnan(grads).all()) and bool(torch.isnan(tail).all()) and bool((ws == 0).all())
    from gmvae_amd.engine import Engine
    e = Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=1, likelihood="gaussian", real_valued=True, likelihood_scale="learned")
    for call in (e.iw_bound_enum_y, e.posterior_y):
        with pytest.raises(ValueError, match="likelihood"):
            call(xd.view(B, d.D), 4)
    with pytest.raises(ValueError, match="float"):
        e.step(torch.zeros(B, d.D, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="finite"):
        e.step(torch.full((B, d.D), float("nan"), device="cuda"))
    with pytest.raises(ValueError, match="learned"):
        e.set_likelihood_sigma(0.5)
    with pytest.raises(ValueError, match="binarises"):
        e.capture_train_pipeline(None, B, lr=LR_, n_steps=2)


# 9 --------------------------------------------------------------------------------------------------------------
def test_model_api_on_floats():
    import torch
    from gmvae_amd import gmvae
    d = O.Dims(D=100, L=5, K=7, hidden=(24,), sigma_min=0.001, raw_sigma_bias=0.25)
    model, B = O.MODEL_GMVAE, 8
    m = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=4,
                           likelihood="gaussian", likelihood_sigma=0.5, real_valued=True, likelihood_scale="learned")
    e = m._engine
    x, rho32 = RR.real_batch(B, d.D, seed=31)
    with torch.no_grad():
        e.views()["decoder/log_sigma"].copy_(torch.from_numpy(rho32))
    _, eps, u = O.make_inputs(d, B, model)
    xt = torch.from_numpy(x).cuda()
    loss = m.run_model(xt, xt, eps=torch.from_numpy(eps).cuda(), u=torch.from_numpy(u).cuda())
    flat = e.params.detach().cpu().numpy().astype(np.float64)
    P0 = e.P - RR.pad4(d.D)
    assert np.array_equal(flat[P0:P0 + d.D], rho32.astype(np.float64))
    p32 = O.unpack(model, d, flat[:P0])
    Cc, _ = RR.loss_and_grads(model, d, p32, x.astype(np.float64), eps, u, rho=rho32.astype(np.float64))
    assert abs(loss.item() - Cc["loss"]) <= 1e-4 * max(abs(Cc["loss"]), Cc["nll_abs"]), (loss.item(), Cc["loss"])
    s = m.summaries
    assert abs(s["recon_mse"].item() - Cc["sqerr"] / (B * d.D)) <= 1e-4 * Cc["sqerr"] / (B * d.D)
    assert abs(s["sigma_mean"].item() - np.exp(rho32.astype(np.float64)).mean()) <= 1e-5 * np.exp(rho32).mean()
    # the decoder is a Normal with the per-dimension scale
    z = torch.randn(6, d.L, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 3.0
    dist = m.decoder(z)
    assert type(dist).__name__ == "NormalDiagScale" and torch.equal(dist.mean(), dist.loc)
    assert torch.allclose(dist.sigma.cpu(), torch.from_numpy(np.exp(rho32)), rtol=1e-6)
    ref_lp = (-0.5 * ((xt[:6].double().cpu() - dist.loc.double().cpu()) / torch.from_numpy(np.exp(rho32.astype(np.float64)))) ** 2
              - torch.from_numpy(rho32.astype(np.float64)) - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert torch.allclose(dist.log_prob(xt[:6]).double().cpu(), ref_lp, rtol=1e-4)
    # every method of the surface takes the float rows
    rec = m.reconstruct_images(xt)
    assert rec.shape == (B, d.D) and bool(torch.isfinite(rec).all()) and float(rec.abs().max()) > 0
    gen = m.generate_sample_images(num_samples=2)
    assert gen.shape[-1] == d.D and bool(torch.isfinite(gen).all())
    assert bool(torch.isfinite(m.generate_samples(num_samples=3)).all())
    code = m.transform(xt)
    assert code.shape == (B, d.L) and bool(torch.isfinite(code).all())
    enc = m.encode(xt)
    assert enc is not None
    cl = m.predict_clusters(xt)
    assert cl.shape[0] == B and bool(((cl >= 0) & (cl < d.K)).all())
    # the state dict carries rho; a checkpoint without it (or with it, into a fixed-scale model) does not restore
    sd = m.state_dict()
    assert torch.equal(sd["decoder/log_sigma"].cpu(), torch.from_numpy(rho32))
    fixed = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=4,
                               likelihood="gaussian", likelihood_sigma=0.5, real_valued=True)
    assert "decoder/log_sigma" not in fixed.state_dict() and fixed._engine.P == P0
    assert torch.equal(fixed.params.detach(), m.params.detach()[:P0])      # (the same initial parameters in front of rho)
    with pytest.raises(ValueError, match="decoder/log_sigma"):
        fixed.load_state_dict(sd)
    with pytest.raises(ValueError, match="decoder/log_sigma"):
        m.load_state_dict(fixed.state_dict())
    m2 = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=9,
                            likelihood="gaussian", likelihood_sigma=0.5, real_valued=True, likelihood_scale="learned")
    m2.load_state_dict(sd)
    assert torch.equal(m2.params.detach(), m.params.detach())
    # DeviceDataset keeps float rows with binarize=False
    from gmvae_amd.data import DeviceDataset
    ds = DeviceDataset(x, np.arange(B), shuffle=False, binarize=False)
    xb, lb = ds.next_batch(4)
    assert ds.pixels.dtype == torch.float32 and torch.equal(xb.cpu(), torch.from_numpy(x[:4])) and lb.tolist() == [0, 1, 2, 3]


# 10 -------------------------------------------------------------------------------------------------------------
def test_runner_trains_restores_and_evaluates_on_synthetic_real(tmp_path, capsys):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=64", "--max_steps=199", "--summarise_every=50", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=512", "--data_dim=40", "--likelihood=gaussian", "--likelihood_sigma=0.5",
            "--real_valued", "--likelihood_scale=learned", "--standardize", "--learning_rate=0.003"]
    model = run_gmvae.main(["--mode=train"] + args)
    e = model._engine
    assert runners.run_train.last_path == "graph+real" and e.real_valued and e.likelihood_scale == "learned" and e.global_step == 200
    out = capsys.readouterr().out
    assert "recon_mse" in out and "loss:" in out and "cluster_acc" in out
    sd = torch.load(runners._ckpt(run_gmvae.build_parser().parse_args(args)), map_location="cpu")
    assert sd["likelihood"] == "gaussian" and sd["real_valued"] is True and sd["likelihood_scale"] == "learned"
    assert sd["decoder/log_sigma"].shape == (40,) and sd["standardize_mean"].shape == (40,) and sd["standardize_std"].shape == (40,)
    xs, _ = runners.synthetic_real(512, 40)
    assert np.allclose(sd["standardize_mean"].numpy(), xs.mean(axis=0), atol=1e-5)
    # a second run restores the checkpoint bit for bit (and has no step left to take)
    again = run_gmvae.main(["--mode=train"] + args)
    assert "restored" in capsys.readouterr().out and again._engine.global_step == 200
    for u, v in ((model.params, again.params), (e.m, again._engine.m), (e.v, again._engine.v)):
        assert torch.equal(u.detach(), v.detach())
    res = run_gmvae.main(["--mode=eval", "--iw_samples=5"] + args)
    out = capsys.readouterr().out
    assert "train/recon_mse" in out and "train/cluster_acc_q" in out and "train/sigma_mean" in out
    assert res["examples"] == 512 and np.isfinite(res["train/loss_per_example"]) and np.isfinite(res["train/iw_bound_5_per_example"])
    # standardised blobs have unit variance per feature: a trained decoder explains most of it, and the learned scales left 0.5
    assert 0.0 < res["train/recon_mse"] < 0.5 and 0.0 < res["train/sigma_mean"] < 1.0 and res["train/sigma_mean"] != 0.5
    assert 0.1 <= res["train/cluster_acc_q"] <= 1.0
    # restoring without --real_valued, or under the fixed scale, is an error
    for drop in ("--real_valued", "--likelihood_scale=learned"):
        other = [a for a in args if a != drop and a != "--standardize"]
        with pytest.raises((ValueError, SystemExit), match="cannot be restored"):
            run_gmvae.main(["--mode=eval"] + other)
