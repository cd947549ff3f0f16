"""Count data under the Poisson and the negative-binomial decoder (GMVAE_LIK_POISSON, GMVAE_LIK_NEG_BINOMIAL) on the device: the
step through the C ABI on explicit noise against the fp64 statement (tests/count_ref.py) at the project's standing gates -- the
loss at 1e-4 of max(|loss|, nll_abs), nll at 1e-4 of nll_abs, kl / nent at 1e-4 of max(|.|, 1), every gradient tensor (rho's
included) at 1e-4 of its own max, tail[5] at 1e-4 relative to itself, tail[6..7] exact (test_lik.lik_gates / sq_gates,
hip_util.check_grads) --, the three tile forms under the forced configurations of tests/epilogue_cases.py, the saturated case,
one TF-Adam step element by element, the bit-for-bit identities (two runs; eager, 1-step graph, n-step graph), gmvae_iw_bound,
the refusals, the bytes-owned contract on the new workspace regions, and 200 steps on runners.synthetic_counts.

The saturated case (lambda over about +-30, rho in {-5, 0, 8}, x from 0 to 1e4) is held to the standing gates too: measured on
an MI355X every figure sits inside them, so no allowance is taken.  The test still prints, beside each error, 4x what the fp64
statement moves when its parameters are perturbed by one fp32 ulp (saturated_allowance): what the conditioning of the inputs
alone would cost (profiles/count_notes.md records the figures)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import adam_ref as AR
import arena as A
import count_ref as CR
import epilogue_cases as EC
import oracle as O
from hip_util import _L, check_grads, dev, device_masks, dims_of, exact_workspace, out, pitch_of, put, put_x, run_checked, workspace
from test_count_cpu import refusals
from test_lik import lik_gates, sq_gates

pytestmark = pytest.mark.gpu

SEED, STEP = 11, 3
_REF = {}          # key -> the fp64 statement's (C, g): computed once, shared, left unchanged


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _cdims(d, B, fl):
    cd = dims_of(d, B)
    cd.sched_flags = fl
    return cd


def cstep(model, d, flat, x, eps, u, fl, seed=5, step=3, row0=0):
    """One gmvae_step at row0 under the flags (x float32): (grad sums [P] float64, tail [8], the step's ReLU masks, the buffer's
    bits)."""
    import torch
    L = _L()
    B = x.shape[0]
    cd = _cdims(d, B, fl)
    cd.row0 = row0
    P, _ = L.param_count(cd, model)
    assert P == flat.shape[0]
    params, xd = dev(flat, torch.float32), dev(x, torch.float32)
    ed = None if eps is None else dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    ws = workspace(cd, model)
    L.check(L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws), seed, step,
                             None, L.current_stream()), "gmvae_step")
    torch.cuda.synchronize()
    g = grads.cpu().numpy().astype(np.float64)
    return g[:P], g[P:], device_masks(ws, cd, model, d, B), grads.cpu()


def _rho_gate(what, gs, g, flat, D, B, rtol=1e-4):
    P0 = flat.shape[0] - CR.pad4(D)
    got, ref = gs[P0:P0 + D] / B, g[CR.LOG_DISPERSION]
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
    print(f"{what} {CR.LOG_DISPERSION}: rel-to-max err {err:.3e}")
    assert err <= rtol, (what, err)
    assert not gs[P0 + D:].any()                                # (the pad behind rho's D values)


def _hold(what, kind, model, d, p32, flat, x, eps, u, rho, gs, tail, masks, Cc, g):
    B, D = x.shape[0], d.D
    assert np.isfinite(gs).all() and np.isfinite(tail).all()
    lik_gates(what, tail, B, Cc)
    sq_gates(what, tail, B, D, Cc)
    check_grads(what, model, d, gs, g, B, masks, Cc["pre"],
                lambda mk: CR.loss_and_grads(model, d, p32, x, eps, u, kind, rho, relu_masks=mk)[1])
    if kind == "nb":
        _rho_gate(what, gs, g, flat, D, B)


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CR.VARIANTS)
def test_step_matches_fp64_statement(name, kind):
    model, d, p32, flat, x, eps, u, rho = CR.setup(name, kind)
    B = x.shape[0]
    L = _L()
    assert L.step_schedule(_cdims(d, B, CR.FLAG[kind]), model) == "general" + CR.SUFFIX[kind]
    gs, tail, masks, _ = cstep(model, d, flat, x, eps, u, CR.FLAG[kind])
    Cc, g = _ref((name, kind), lambda: CR.loss_and_grads(model, d, p32, x, eps, u, kind, rho))
    _hold(f"{name}-{kind}", kind, model, d, p32, flat, x, eps, u, rho, gs, tail, masks, Cc, g)


# 2 --------------------------------------------------------------------------------------------------------------
def _tile_case(shape, kind):
    sh = EC.SHAPES[shape]
    model, d, B = O.MODEL_NAMES[sh.mname], sh.d, sh.B
    rng = np.random.default_rng(B)
    p = O.init_params(model, d, rng)
    _, eps, u = O.make_inputs(d, B, model)
    u = u if model == O.MODEL_GMVAE else None
    x, rho32 = CR.count_batch(B, d.D)
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    rho = None
    if kind == "nb":
        flat, rho = CR.with_rho(flat, rho32, d.D), rho32.astype(np.float64)
    return model, d, p32, flat, x, eps, u, rho


@pytest.mark.parametrize("kind", CR.KINDS)
@pytest.mark.parametrize("shape", ["whole", "ragged", "unaligned"])
def test_every_tile_form_runs_the_count_branch(shape, kind, monkeypatch):
    """epilogue_cases' shapes under GMVAE_FORCE_CFG = 0, 1, 2: interior tiles, the quad-predicated last column tile, ragged rows
    and unaligned rows in each of the three tile configurations, each at the standing gates; the three gradient buffers are
    pairwise not bit-identical (a forced configuration ran)."""
    import torch
    model, d, p32, flat, x, eps, u, rho = _tile_case(shape, kind)
    R = x.shape[0] * d.S
    Cc, g = _ref((shape, kind), lambda: CR.loss_and_grads(model, d, p32, x, eps, u, kind, rho))
    seen = []
    for cfg in EC.CFGS:
        for k in ("GMVAE_FORCE_CFG", "GMVAE_NO_BIG", "GMVAE_NO_PLANES", "GMVAE_NSPLIT_SMALL"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("GMVAE_FORCE_CFG", str(cfg))
        assert EC.tile_paths(R, d.D, *EC.TILE[cfg])
        gs, tail, masks, bits = cstep(model, d, flat, x, eps, u, CR.FLAG[kind])
        _hold(f"{shape}-{kind}-cfg{cfg}", kind, model, d, p32, flat, x, eps, u, rho, gs, tail, masks, Cc, g)
        seen.append(bits)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


# 3 --------------------------------------------------------------------------------------------------------------
def saturated_allowance(model, d, p32, x, eps, u, kind, rho, Cc, g):
    """What the fp64 statement moves when every parameter (rho too) is perturbed by one fp32 ulp, times 4: what the conditioning
    of the inputs alone costs any fp32 evaluation.  Printed beside each error, never asserted on.  {name: absolute figure}."""
    rng = np.random.default_rng(1)
    bump = lambda a: (a.astype(np.float32) + np.spacing(np.abs(a).astype(np.float32)) * rng.choice([-1.0, 1.0], a.shape).astype(np.float32)).astype(np.float64)
    p2 = {k: bump(v) for k, v in p32.items()}
    r2 = None if rho is None else bump(rho)
    C2, g2 = CR.loss_and_grads(model, d, p2, x, eps, u, kind, r2)
    al = {k: 4 * abs(C2[k] - Cc[k]) for k in ("loss", "nll", "kl", "nent", "sqerr")}
    al.update({k: 4 * np.abs(g2[k] - g[k]).max() for k in g})
    return al


@pytest.mark.parametrize("kind", CR.KINDS)
@pytest.mark.parametrize("name", ["gmvae-b32-d100-s3", "vae-b5-d13-s3"])
def test_saturated_case(name, kind):
    """lambda over about +-30, rho cycling through -5, 0, 8, x from 0 to 1e4: finite everywhere, and every figure inside its
    standing gate."""
    model, d, p32, flat, x, eps, u, rho = CR.setup(name, kind, saturated=True)
    B, D = x.shape[0], d.D
    Cc, g = _ref((name, kind, "sat"), lambda: CR.loss_and_grads(model, d, p32, x, eps, u, kind, rho))
    assert np.abs(Cc["lam"]).max() > 20
    gs, tail, masks, _ = cstep(model, d, flat, x, eps, u, CR.FLAG[kind])
    assert np.isfinite(gs).all() and np.isfinite(tail).all()
    al = saturated_allowance(model, d, p32, x, eps, u, kind, rho, Cc, g)
    what = f"{name}-{kind}-saturated"
    gates = {"loss": 1e-4 * max(abs(Cc["loss"]), Cc["nll_abs"]), "nll": 1e-4 * Cc["nll_abs"], "kl": 1e-4 * max(abs(Cc["kl"]), 1.0),
             "nent": 1e-4 * max(abs(Cc["nent"]), 1.0), "sqerr": 1e-4 * abs(Cc["sqerr"])}
    got = {"loss": tail[0] / B, "nll": tail[1] / B, "kl": tail[2] / B, "nent": tail[3] / B, "sqerr": tail[5]}
    for k in gates:
        err = abs(got[k] - Cc[k])
        print(f"{what} {k}: err {err:.3e} gate {gates[k]:.3e} allowance {al[k]:.3e}")
    lay, _, _ = O.param_layout(model, d)
    P0 = flat.shape[0] - CR.pad4(D)
    tensors = [(n, gs[o:o + int(np.prod(s))].reshape(s) / B, g[n]) for n, s, o in lay]
    if kind == "nb":
        tensors.append((CR.LOG_DISPERSION, gs[P0:P0 + D] / B, g[CR.LOG_DISPERSION]))
    gerr = []
    for n, a, r in tensors:
        err, gate = np.abs(a - r).max(), 1e-4 * max(np.abs(r).max(), 1e-6)
        print(f"{what} {n}: err {err:.3e} gate {gate:.3e} allowance {al[n]:.3e}")
        gerr.append((n, err, gate))
    assert tail[4] == B and tail[6] == B * D and tail[7] == 0
    for k in gates:
        assert abs(got[k] - Cc[k]) <= gates[k], (what, k)
    for n, err, bound in gerr:
        assert err <= bound, (what, n, err, bound)


# 4 --------------------------------------------------------------------------------------------------------------
def _engine(mname, d, seed, lik, **kw):
    from gmvae_amd.engine import Engine
    return Engine(mname, d.D, d.L, d.K, list(d.hidden), n_samples=d.S, random_seed=seed, temperature=d.temperature,
                  sigma_min=d.sigma_min, likelihood=lik, **kw)


def _batches(d, B, n, seed):
    import torch
    return torch.from_numpy(np.stack([CR.count_batch(B, d.D, seed=seed + i)[0] for i in range(n)])).cuda()


@pytest.mark.parametrize("kind", CR.KINDS)
def test_one_optimizer_step_element_by_element(kind):
    """Every parameter (rho among them), m and v after an eager TF-Adam step against the update statement (tests/adam_ref.py) on
    the step's own gradient sums, element by element, as tests/test_optimizer_sites.py holds its sites."""
    import torch
    c = CR.CASES["gmvae-b32-d100-s3"]
    d, B = c.d, c.B
    e = _engine("gmvae", d, 7, CR.NAME[kind])
    assert e.real_valued and (kind != "nb" or e.layout[-1][0] == CR.LOG_DISPERSION)
    xs = _batches(d, B, 2, 20)
    hp = AR.HP[1]
    for i in range(2):
        p0, m0, v0 = (t.detach()[:e.P].cpu().numpy() for t in (e.params, e.m, e.v))
        e.train_step(xs[i], lr=hp[0])
        torch.cuda.synchronize()
        gsum, count = e.grads[:e.P].cpu().numpy(), e.grads[e.P + 4].item()
        assert count == B and np.isfinite(gsum).all() and np.abs(gsum).max() > 0
        want = AR.predict(p0, m0, v0, gsum, count, i + 1, *hp)
        dm, dv, dp = AR.bounds(p0, m0, v0, gsum, count, i + 1, *hp)
        for what, got, ref, bound in (("p", e.params.detach()[:e.P], want[0], dp), ("m", e.m[:e.P], want[1], dm), ("v", e.v[:e.P], want[2], dv)):
            r, j = AR.worst(got.cpu().numpy(), ref, bound)
            print(f"{kind} step {i + 1} {what}: worst error / bound {r:.3f} at {j}")
            assert r <= 1.0, (kind, i, what, r, j)
    if kind == "nb":
        rho = e.views()[CR.LOG_DISPERSION]
        assert bool((rho != 0).all())                           # (rho moved off its initial 0)


# 5 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("gmvae-b32-d100-s3", "nb"), ("vae-b5-d13-s3", "nb"), ("vae_gmp-b32-d128-s1", "poisson")])
def test_two_runs_are_bit_equal(name, kind):
    import torch
    model, d, p32, flat, x, eps, u, rho = CR.setup(name, kind)
    a = cstep(model, d, flat, x, eps, u, CR.FLAG[kind])[3]
    b = cstep(model, d, flat, x, eps, u, CR.FLAG[kind])[3]
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("mname,kind,clip", [("gmvae", "nb", None), ("vae", "nb", 0.5), ("vae_gmp", "poisson", None)])
def test_eager_one_step_graph_and_n_step_graph_agree(mname, kind, clip):
    """Three eager steps, three replays of a 1-step graph and one replay of a 3-step graph end on the same bits: parameters (rho
    among them), m, v and the tails."""
    import torch
    d, B = CR._dims(mname, 100, 3), 16
    xs = _batches(d, B, 3, 8)
    kw = dict(clip_norm=clip) if clip else {}
    a, b, c = (_engine(mname, d, 11, CR.NAME[kind], **kw) for _ in range(3))
    tails = [a.train_step(xs[t], lr=1e-3).clone() for t in range(3)]
    s1, r1 = b.capture_train_step(B, lr=1e-3, n_steps=1)
    assert s1.dtype == torch.float32
    for t in range(3):
        s1.copy_(xs[t])
        r1()
    s3, r3 = c.capture_train_step(B, lr=1e-3, n_steps=3)
    s3.copy_(xs)
    r3()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == c.global_step == 3
    for o in (b, c):
        for u, v in ((a.params, o.params), (a.m, o.m), (a.v, o.v)):
            assert torch.equal(u.detach(), v.detach())
    assert torch.equal(r3.tail_log, torch.stack(tails))
    tl = r3.tail_log.cpu()
    assert bool(torch.isfinite(tl).all()) and bool((tl[:, 5] > 0).all()) and bool((tl[:, 6] == B * d.D).all()) and bool((tl[:, 7] == 0).all())


# 6 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("vae-b5-d13-s3", "poisson"), ("gmvae-b5-d100-s1", "nb"), ("vae_gmp-b5-d128-s3", "nb")])
def test_iw_bound(name, kind):
    """n = 7 in chunks of 3 against the statement on the regenerated noise (Philox row (row0 + b) n + s)."""
    import torch
    L = _L()
    n, chunk = 7, 3
    model, d, p32, flat, x, eps, u, rho = CR.setup(name, kind)
    B = x.shape[0]
    ref, mag = [], []
    for b in range(B):
        e, uu = O.noise(n, d.L, d.K, b * n, SEED, STEP)
        Cb, _ = CR.loss_and_grads(model, dataclasses.replace(d, S=n), p32, x[b:b + 1], e, uu if model == O.MODEL_GMVAE else None, kind, rho)
        ref.append(Cb["bound"][0])
        mag.append(Cb["nll_abs"])
    ref, mag = np.array(ref), np.array(mag)
    cd = _cdims(dataclasses.replace(d, S=chunk), B, CR.FLAG[kind])
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    bound, mlw = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.float32)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, L.ptr(bound), L.ptr(mlw), L.ptr(tail), L.ptr(ws),
                                 SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    bound, mlw, tail = bound.cpu().numpy(), mlw.cpu().numpy(), tail.cpu().numpy()
    print(f"{name}-{kind}: bound {bound.tolist()} ref {ref.tolist()}")
    gate = 1e-4 * np.maximum(np.maximum(np.abs(ref), mag), 1.0)
    assert np.all(np.abs(bound - ref) <= gate), (bound, ref)
    assert np.all(mlw <= bound + gate)
    assert tail[4] == B and (tail[5:] == 0).all()


# 7 --------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch():
    """Every refusal by its code with host dummies for every pointer (a launch would fault on them), an unaligned x included."""
    refusals(_L())


# 8 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("gmvae-b32-d100-s3", "nb"), ("vae-b5-d13-s3", "nb"), ("vae_gmp-b5-d128-s3", "poisson")])
def test_step_stays_inside_the_bytes_its_caller_owns(name, kind):
    """tests/test_memory_contract.py's contract on the new workspace regions: x at exactly 4 B D bytes and the parameters read-only,
    the gradient buffer and a workspace of exactly gmvae_workspace_bytes writable -- t, the partials, c, sp(u) and the fp64 slab
    partials lie at its end --, guard bands around each; the guarded step gives the unguarded step's bits."""
    import torch
    L = _L()
    model, d, p32, flat, x, eps, u, rho = CR.setup(name, kind)
    B = x.shape[0]
    ar = A.Arena("cuda", 1 << 25)
    cd = dims_of(d, B, ar)
    cd.sched_flags = CR.FLAG[kind]
    P, _ = L.param_count(cd, model)
    pitch = pitch_of(d)
    params = put(ar, "params", flat, torch.float32, pitch)
    xd = put_x(ar, x, d.D)
    ed = put(ar, "eps", eps, torch.float32, 4 * d.L)
    ud = None if u is None else put(ar, "u", u, torch.float32, 4 * d.K)
    grads = out(ar, "grads", (P + L.TAIL,), pitch)
    ws = exact_workspace(ar, L.workspace_bytes(cd, model), pitch)
    run_checked(ar, "gmvae_step", lambda: L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params),
                                                           L.ptr(grads), L.ptr(ws), 5, 3, None, L.current_stream()))
    plain = cstep(model, d, flat, x, eps, u, CR.FLAG[kind])[3]
    assert bool(torch.isfinite(plain).all()) and torch.equal(grads.cpu(), plain)


# 9 --------------------------------------------------------------------------------------------------------------
def test_nb_gmvae_learns_synthetic_counts():
    """200 steps of the negative-binomial GMVAE on runners.synthetic_counts (N = 512, D = 100, K = 3) lower the loss, and the
    clustering accuracy of q(y|x) beats the same run's step-0 value."""
    import torch
    from gmvae_amd import create_gmvae, runners, utils
    x, lab = runners.synthetic_counts(512, 100, 3)
    xt, lt = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    model = create_gmvae(100, 8, mixture_components=3, fcnet_hidden_sizes=[64], random_seed=3, likelihood="negative_binomial")
    e = model._engine
    acc = lambda: utils.cluster_acc(model.encoder_y(xt).distribution.logits, lt, 3).item()
    acc0 = acc()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    losses = []
    for i in range(200):
        idx = torch.randperm(512, device="cuda", generator=gen)[:128]
        losses.append(e.train_step(xt[idx], lr=3e-3)[0].item() / 128)
    acc1 = acc()
    first, last = np.mean(losses[:10]), np.mean(losses[-10:])
    print(f"loss {first:.2f} -> {last:.2f}; cluster_acc {acc0:.3f} -> {acc1:.3f}; dispersion_mean {torch.exp(e.views()[CR.LOG_DISPERSION]).mean().item():.3f}")
    assert np.isfinite(losses).all() and last < first
    assert acc1 > acc0
    # the model API on the trained model: summaries, the importance-weighted bound, the decoder's distribution and its mean
    s = model.summaries
    assert abs(s["dispersion_mean"].item() - torch.exp(e.views()[CR.LOG_DISPERSION]).mean().item()) < 1e-6 and s["recon_mse"].item() > 0
    xb = xt[:16]
    b1, b64 = model.iw_bound(xb, 1), model.iw_bound(xb, 64, chunk=16)
    assert bool(torch.isfinite(b64).all()) and b64.mean().item() > b1.mean().item() - 1.0      # (more samples: a tighter bound)
    z = torch.randn(16, 8, device="cuda")
    dist = model.decoder(z)
    from gmvae_amd import base
    assert isinstance(dist, base.NegativeBinomial) and bool((dist.mean() > 0).all()) and bool(torch.isfinite(dist.log_prob(xb)).all())
    with pytest.raises(ValueError, match="counts"):
        e.step(-xb)


# 10 -------------------------------------------------------------------------------------------------------------
def test_runner_trains_restores_and_evaluates_on_a_count_file(tmp_path, capsys):
    """run_gmvae --likelihood negative_binomial --data_npy --labels_npy: a captured train graph on float count batches, the
    options in the checkpoint, a bit-for-bit restore, eval with the importance-weighted bound; a Poisson run cannot restore it."""
    import torch
    from gmvae_amd import run_gmvae, runners
    x, lab = runners.synthetic_counts(512, 40, 3)
    np.save(tmp_path / "counts.npy", x)
    np.save(tmp_path / "labels.npy", lab)
    args = ["--model=gmvae", "--latent_size=8", "--mixture_components=3", "--batch_size=64", "--max_steps=99", "--summarise_every=50",
            f"--logdir={tmp_path}", "--random_seed=1", "--likelihood=negative_binomial", f"--data_npy={tmp_path / 'counts.npy'}",
            f"--labels_npy={tmp_path / 'labels.npy'}", "--learning_rate=0.003"]
    model = run_gmvae.main(["--mode=train"] + args)
    e = model._engine
    assert runners.run_train.last_path == "graph+real" and e.real_valued and e.likelihood == "negative_binomial" and e.global_step == 100
    out = capsys.readouterr().out
    assert "recon_mse" in out and "loss:" in out and "cluster_acc" in out
    sd = torch.load(runners._ckpt(run_gmvae.build_parser().parse_args(args)), map_location="cpu")
    assert sd["likelihood"] == "negative_binomial" and sd["real_valued"] is True and sd[CR.LOG_DISPERSION].shape == (40,)
    assert bool((sd[CR.LOG_DISPERSION] != 0).all())
    again = run_gmvae.main(["--mode=train"] + args)
    assert "restored" in capsys.readouterr().out and again._engine.global_step == 100
    for u, v in ((model.params, again.params), (e.m, again._engine.m), (e.v, again._engine.v)):
        assert torch.equal(u.detach(), v.detach())
    res = run_gmvae.main(["--mode=eval", "--iw_samples=5"] + args)
    out = capsys.readouterr().out
    assert "train/recon_mse" in out and "train/cluster_acc_q" in out and "train/dispersion_mean" in out
    assert res["examples"] == 512 and np.isfinite(res["train/loss_per_example"]) and np.isfinite(res["train/iw_bound_5_per_example"])
    assert res["train/dispersion_mean"] > 0 and 0.3 <= res["train/cluster_acc_q"] <= 1.0
    other = [a.replace("negative_binomial", "poisson") for a in args]
    with pytest.raises((ValueError, SystemExit), match="cannot be restored"):
        run_gmvae.main(["--mode=eval"] + other)
