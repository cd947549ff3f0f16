"""Gradient clipping by the global norm (GMVAE_OPT_CLIP_NORM) on the device: gmvae_grad_clip on synthetic buffers against the
fp64 statement (tests/clip_ref.py), the eager step, the train graphs, the pipeline graph and the one-rank data-parallel forms
-- all the same bits --, set_clip_norm between replays, the skips, and run_train's log.

Figures of one run on an MI355X (worst |device - fp64| / bound; the bound is 2 u of the value, clip_ref):
  gmvae_grad_clip, synthetic buffers: 0.35 / 0.36 / 0.41 / 0.44 / 0.33 / 0.42 at P = 4 / 1020 / 1024 / 1028 / 166620 / 2^20 + 4
    (the one rounding to fp32 can take 0.5; the fp64 sum's own error is below 1e-8 of the bound)
  eager train_step: the record 0.30 or below; (p', m', v') inside adam_ref.bounds with count := d, worst p' 0.17, m' 0.06, v' 0.001
  (profiles/clip_notes.md has the table)"""
import ctypes as C
import math

import numpy as np
import pytest

import adam_ref
import clip_ref

pytestmark = pytest.mark.gpu

LR = 1e-3
HP = (1e-3, 0.9, 0.999, 1e-8)


def _L():
    from gmvae_amd import _lib
    return _lib


def _default_P():
    L = _L()
    return L.param_count(L.make_dims(1, 784, 64, 10, (64,)), L.MODEL_GMVAE)[0]


def _grad_clip(buf_dev, P, C_value, scratch=None):
    """One call of gmvae_grad_clip: the record [4] as numpy (after a sync)."""
    import torch
    L = _L()
    cn = torch.tensor([C_value], dtype=torch.float32).cuda()
    rec = torch.full((4,), -7.0, dtype=torch.float32).cuda()
    if scratch is None:
        scratch = torch.zeros(L.grad_clip_scratch_bytes(P) // 8, dtype=torch.float64).cuda()
    L.check(L.lib.gmvae_grad_clip(L.ptr(buf_dev), P, L.ptr(cn), L.ptr(rec), L.ptr(scratch), L.current_stream()), "gmvae_grad_clip")
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _buffer(P, g, count, loss=-12.5):
    b = np.zeros(P + clip_ref.TAIL, dtype=np.float32)
    b[:P] = g
    b[P], b[P + 4] = loss, count
    return b


# ------------------------------------------------------------------ 1. the entry point on synthetic buffers
@pytest.mark.parametrize("P", [4, 1020, 1024, 1028, "default", 2 ** 20 + 4])
def test_grad_clip_on_synthetic_buffers(P):
    import torch
    P = _default_P() if P == "default" else P
    rng = np.random.default_rng(P)
    worst = 0.0
    unit = rng.standard_normal(P).astype(np.float32)
    for scale in (1e-3, 1.0, 1e3):
        for count in (1.0, 100.0, 1024.0):
            b = _buffer(P, unit * np.float32(scale), count)
            dev = torch.from_numpy(b).cuda()
            norm = clip_ref.record(b, math.inf)[0]
            for ratio in (0.01, 0.5, 0.998, 1.002, 10.0, math.inf):
                Cv = float(np.float32(ratio * norm))
                assert not clip_ref.flag_band(b, Cv)
                rec = _grad_clip(dev, P, Cv)
                worst = max(worst, clip_ref.check_record(rec, b, Cv))
                assert bool(rec[2]) == (ratio < 1)
            rec2 = _grad_clip(dev, P, Cv)
            assert np.array_equal(rec.view(np.uint32), rec2.view(np.uint32))       # two calls: the same bits
    # ---- special buffers
    ones = np.ones(P, dtype=np.float32)
    specials = {}
    specials["zeros"] = (_buffer(P, 0.0, 16.0), 1.0)
    big = ones.copy()
    big[P // 2] = 3e19                                  # its square overflows fp32
    specials["3e19"] = (_buffer(P, big, 16.0), 1.0)
    specials["1e-25"] = (_buffer(P, np.float32(1e-25), 1.0), 1.0)           # every square is 0 in fp32
    for name, v in (("nan", math.nan), ("inf", math.inf)):
        g = ones.copy()
        g[P - 1] = v
        specials[name] = (_buffer(P, g, 16.0), 1.0)
    specials["nan-loss"] = (_buffer(P, ones, 16.0, loss=math.nan), 1.0)
    specials["C=0"] = (_buffer(P, ones, 16.0), 0.0)
    specials["C<0"] = (_buffer(P, ones, 16.0), -1.0)
    specials["C=nan"] = (_buffer(P, ones, 16.0), math.nan)
    edge = np.zeros(P, dtype=np.float32)                # non-zero words at the last block's edges only: a short last block
    last0 = (P - 1) // 1024 * 1024
    for i in {last0, P - 4, P - 1, max(last0 - 1, 0)}:
        edge[i] = 3.0 + i % 5
    specials["edge"] = (_buffer(P, edge, 4.0), 0.25)
    for name, (b, Cv) in specials.items():
        rec = _grad_clip(torch.from_numpy(b).cuda(), P, Cv)
        worst = max(worst, clip_ref.check_record(rec, b, Cv))
        skip = clip_ref.record(b, Cv)[3]
        assert skip == (name in ("nan", "inf", "nan-loss", "C=0", "C<0", "C=nan")), name
        if not skip:
            assert np.isfinite(rec).all(), (name, rec)
    assert _grad_clip(torch.from_numpy(specials["zeros"][0]).cuda(), P, 1.0).tolist() == [0.0, 16.0, 0.0, -12.5]
    assert _grad_clip(torch.from_numpy(specials["edge"][0]).cuda(), P, 0.25)[2] == 1.0
    print(f"\n[clip] gmvae_grad_clip P={P}: worst |device - fp64| / bound = {worst:.3f}")


# ------------------------------------------------------------------ engines
CASES = {
    "gmvae-small": dict(model="gmvae", D=20, Lz=4, K=3, hidden=(8,), B=5, kw={}),
    "vae-784": dict(model="vae", D=784, Lz=2, K=1, hidden=(64,), B=16, kw={}),
    "vae_gmp-24x24": dict(model="vae_gmp", D=36, Lz=6, K=4, hidden=(24, 24), B=9, kw={}),
    "gmvae-marginal_iw-labels-dreg": dict(model="gmvae", D=20, Lz=4, K=3, hidden=(8,), B=5,
                                          kw=dict(n_samples=2, y_inference="marginal_iw", grad_estimator="dreg", semi_supervised=True)),
}
BIG = dict(model="gmvae", D=100, Lz=8, K=5, hidden=(64, 64), B=40, kw={})      # (takes the general schedule without the option)
ALL = dict(CASES, big=BIG)


def _engine(case, clip_norm, seed=5):
    from gmvae_amd.engine import Engine
    c = ALL[case]
    return Engine(c["model"], c["D"], c["Lz"], c["K"], list(c["hidden"]), random_seed=seed, clip_norm=clip_norm, **c["kw"])


def _batch(case, n=1, seed=1):
    import torch
    c = ALL[case]
    x = torch.from_numpy((np.random.default_rng(seed).random((n, c["B"], c["D"])) < 0.6).astype(np.uint8)).cuda()
    return x if n > 1 else x[0]


def _step_args(case):
    import torch
    if "semi_supervised" not in CASES[case]["kw"]:
        return {}
    return dict(y_observed=torch.tensor([0, -1, 2, -1, 1], dtype=torch.int32).cuda())


def _state(e):
    return [t.detach().clone() for t in (e.params, e.m, e.v)]


def _same(a, b):
    import torch
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu()


# ------------------------------------------------------------------ 2. one eager train_step
@pytest.mark.parametrize("case", list(CASES))
def test_eager_train_step_is_the_statement(case):
    import torch
    L = _L()
    x, args = _batch(case), _step_args(case)
    probe = _engine(case, math.inf)
    assert L.step_schedule(probe.dims(CASES[case]["B"]), probe.model).endswith("+clip")
    probe.train_step(x, lr=LR, **args)
    torch.cuda.synchronize()
    norm0 = float(probe.grad_clip[0])
    assert math.isfinite(norm0) and norm0 > 0 and float(probe.grad_clip[2]) == 0.0
    pad = np.ones(probe.P, dtype=bool)
    for _, (rows, cols), off in probe.layout:
        pad[off:off + rows * cols] = False
    for ratio, want_clipped in ((0.5, 1.0), (2.0, 0.0)):
        Cv = float(np.float32(ratio * norm0))
        e = _engine(case, Cv)
        assert e.noise_seed == probe.noise_seed
        p0, m0, v0 = (t.cpu().numpy() for t in _state(e))
        tail = e.train_step(x, lr=LR, **args)
        torch.cuda.synchronize()
        buf, rec = e.grads.cpu().numpy(), e.grad_clip.cpu().numpy()
        assert float(tail[4]) == CASES[case]["B"] and e.global_step == 1
        w_rec = clip_ref.check_record(rec, buf, Cv)
        assert rec[2] == want_clipped and abs(rec[0] - norm0) <= 4 * clip_ref.U * norm0
        assert not buf[:e.P][pad].any()                                     # the padding words count towards SS: they are zero
        gsum, d = buf[:e.P], np.float64(rec[1])
        ref = adam_ref.predict(p0, m0, v0, gsum, d, 1, *HP)
        bnd = adam_ref.bounds(p0, m0, v0, gsum, d, 1, *HP)
        got = [t.cpu().numpy() for t in _state(e)]
        w = [adam_ref.worst(got[i], ref[j], bnd[k])[0] for i, j, k in ((0, 0, 2), (1, 1, 0), (2, 2, 1))]
        print(f"\n[clip] eager {case} ratio {ratio}: record {w_rec:.3f}, p' {w[0]:.3f} m' {w[1]:.3f} v' {w[2]:.3f} (padding words: "
              f"{int(pad.sum())}, all zero)")
        assert max(w) <= 1.0, w
    from gmvae_amd import gmvae
    if case == "gmvae-small":                                               # the factory and the summaries
        c = CASES[case]
        mdl = gmvae.create_gmvae(c["D"], c["Lz"], mixture_components=c["K"], fcnet_hidden_sizes=list(c["hidden"]), sigma_min=0.0,
                                 raw_sigma_bias=0.5, random_seed=5, clip_norm=0.5 * norm0)
        mdl._engine.train_step(x, lr=LR)
        sm = mdl.summaries
        assert float(sm["clipped"]) == 1.0 and abs(float(sm["grad_norm"]) - norm0) <= 4 * clip_ref.U * norm0


# ------------------------------------------------------------------ 3. a huge threshold changes nothing

def test_huge_threshold_is_the_step_without_the_option():
    import torch
    L = _L()
    xs = _batch("big", 3)
    plain, clip = _engine("big", None), _engine("big", 1e30)
    assert L.step_schedule(plain.dims(40), plain.model) == "general"
    for i in range(3):
        ta, tb = plain.train_step(xs[i], lr=LR).clone(), clip.train_step(xs[i], lr=LR).clone()
        assert torch.equal(_bits(ta), _bits(tb))
        assert float(clip.grad_clip[2]) == 0.0 and float(clip.grad_clip[1]) == 40.0
    assert _same(_state(plain), _state(clip))
    plain, clip = _engine("big", None), _engine("big", 1e30)
    outs = []
    for e in (plain, clip):
        sx, rp = e.capture_train_step(40, lr=LR, n_steps=3)
        sx.copy_(xs)
        rp()
        torch.cuda.synchronize()
        outs.append((_state(e), rp.tail_log.clone(), rp.grad_clip))
    assert outs[0][2] is None and outs[1][2].shape == (3, 4)
    assert _same(outs[0][0], outs[1][0]) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert (outs[1][2][:, 2] == 0).all() and (outs[1][2][:, 1] == 40).all() and torch.isfinite(outs[1][2]).all()


# ------------------------------------------------------------------ 4. all forms agree bit for bit
def _clipping_threshold(case, xs):
    """A threshold below the first step's norm and above nothing: every one of the three steps clips."""
    import torch
    probe = _engine(case, math.inf)
    probe.train_step(xs[0], lr=LR, **_step_args(case))
    torch.cuda.synchronize()
    return 0.25 * float(probe.grad_clip[0])


def _eager3(case, Cv, xs):
    import torch
    e = _engine(case, Cv)
    recs, tails = [], []
    for i in range(3):
        tails.append(e.train_step(xs[i], lr=LR, **_step_args(case)).clone())
        recs.append(e.grad_clip.clone())
    torch.cuda.synchronize()
    return e, torch.stack(recs), torch.stack(tails)


@pytest.mark.parametrize("case", ["gmvae-small", "vae_gmp-24x24", "gmvae-marginal_iw-labels-dreg"])
def test_eager_and_graph_forms_agree_bit_for_bit(case):
    import torch
    B = CASES[case]["B"]
    xs = _batch(case, 3)
    Cv = _clipping_threshold(case, xs)
    e, recs, tails = _eager3(case, Cv, xs)
    assert (recs[:, 2] == 1).all() and torch.isfinite(recs).all()
    labels = _step_args(case).get("y_observed")
    g3 = _engine(case, Cv)
    sx, rp = g3.capture_train_step(B, lr=LR, n_steps=3)
    sx.copy_(xs)
    if labels is not None:
        rp.y_observed.copy_(labels.expand(3, -1))
    rp()
    torch.cuda.synchronize()
    assert _same(_state(e), _state(g3)) and torch.equal(_bits(rp.grad_clip), _bits(recs)) and torch.equal(_bits(rp.tail_log), _bits(tails))
    g1 = _engine(case, Cv)
    sx, rp = g1.capture_train_step(B, lr=LR, n_steps=1)
    for i in range(3):
        sx.copy_(xs[i])
        if labels is not None:
            rp.y_observed.copy_(labels.view(1, -1))
        rp()
        torch.cuda.synchronize()
        assert torch.equal(_bits(rp.grad_clip[0]), _bits(recs[i]))
    assert _same(_state(e), _state(g1)) and g1.global_step == g3.global_step == e.global_step == 3
    with pytest.raises(ValueError, match="at most 32 steps"):
        g1.capture_train_step(B, lr=LR, n_steps=33)


def test_pipeline_graph_agrees_with_the_train_graph():
    import torch
    from gmvae_amd.data import DeviceDataset
    case = "vae-784"
    c = CASES[case]
    pix = np.random.default_rng(8).integers(0, 256, (200, c["D"]), dtype=np.uint8)
    a = _engine(case, 1.0)
    rp = a.capture_train_pipeline(DeviceDataset(pix, shuffle=True, seed=21), c["B"], lr=LR, n_steps=3)
    rp()
    torch.cuda.synchronize()
    assert rp.grad_clip.shape == (3, 4) and torch.isfinite(rp.grad_clip).all()
    b = _engine(case, 1.0)
    sx, rb = b.capture_train_step(c["B"], lr=LR, n_steps=3)
    sx.copy_(rp.batches)
    rb()
    torch.cuda.synchronize()
    assert _same(_state(a), _state(b)) and torch.equal(_bits(rp.grad_clip), _bits(rb.grad_clip))
    assert (rp.grad_clip[:, 2] == 1).any()                                 # (the threshold bites: the untrained VAE's norm is above 1)


# ------------------------------------------------------------------ 5. set_clip_norm between two replays
def test_set_clip_norm_between_replays_needs_no_recapture():
    import torch
    case = "gmvae-small"
    B = CASES[case]["B"]
    xs = _batch(case, 2)
    Cv = _clipping_threshold(case, xs)                  # 0.25 x the first norm
    e = _engine(case, 1e6)
    sx, rp = e.capture_train_step(B, lr=LR, n_steps=2)
    sx.copy_(xs)
    rp()
    torch.cuda.synchronize()
    first = rp.grad_clip.clone()
    assert (first[:, 2] == 0).all()
    e.set_clip_norm(Cv)
    sx2, rp2 = e.capture_train_step(B, lr=LR, n_steps=2)
    assert rp2 is rp and sx2 is sx                      # the same handle: no recapture
    rp()
    torch.cuda.synchronize()
    assert (rp.grad_clip[:, 2] == 1).all() and e.global_step == 4
    with pytest.raises(ValueError):
        e.set_clip_norm(0.0)
    with pytest.raises(ValueError):
        _engine(case, None).set_clip_norm(1.0)


# ------------------------------------------------------------------ 6. data parallel behind a one-rank communicator
def _need_rccl():
    """The one narrow precondition of the one-rank communicator test, decided before any work: the RCCL shared library itself
    loads in this process.  Everything after it -- the project's own communicator code included -- fails the test if it fails."""
    L = _L()
    try:
        C.CDLL(L.rccl_path().decode())
    except OSError as e:
        pytest.skip(f"the RCCL shared library does not load here: {e}")


def test_data_parallel_forms_give_the_single_device_bits():
    import torch
    _need_rccl()
    case = "gmvae-small"
    B = CASES[case]["B"]
    xs = _batch(case, 3)
    Cv = _clipping_threshold(case, xs)
    e, recs, tails = _eager3(case, Cv, xs)
    d = _engine(case, Cv)
    d.enable_rccl()
    for i in range(3):
        t = d.dp_step(xs[i], LR).clone()
        torch.cuda.synchronize()
        assert torch.equal(_bits(d.grad_clip), _bits(recs[i])) and torch.equal(_bits(t), _bits(tails[i]))
    assert _same(_state(e), _state(d))
    g = _engine(case, Cv)
    g.enable_rccl()
    sx, rp = g.capture_train_step(B, lr=LR, all_reduce=True, n_steps=3)
    assert g.dp_mode == "rccl-in-hipgraph"
    sx.copy_(xs)
    rp()
    torch.cuda.synchronize()
    assert _same(_state(e), _state(g)) and torch.equal(_bits(rp.grad_clip), _bits(recs)) and torch.equal(_bits(rp.tail_log), _bits(tails))


# ------------------------------------------------------------------ 7. skips
@pytest.mark.parametrize("poison", ["inf-gradient", "nan-loss"])
def test_eager_step_is_skipped_on_a_poisoned_buffer(poison):
    import torch
    case = "gmvae-small"
    e = _engine(case, 1.0)
    e.step(_batch(case))
    if poison == "inf-gradient":
        e.grads[e.P // 2].fill_(math.inf)
    else:
        e.grads[e.P].fill_(math.nan)
    before = _state(e)
    e.adam(LR)
    torch.cuda.synchronize()
    assert _same(before, _state(e)) and math.isnan(float(e.grad_clip[3])) and e.global_step == 1 and int(e.step_dev[0]) == 1
    e.train_step(_batch(case), lr=LR)                   # the next step applies
    torch.cuda.synchronize()
    assert not _same(before, _state(e)) and math.isfinite(float(e.grad_clip[3])) and e.global_step == 2


def test_zero_threshold_in_the_workspace_cell_skips_every_step():
    import torch
    L = _L()
    case = "gmvae-small"
    B = CASES[case]["B"]
    e = _engine(case, 1.0)
    sx, rp = e.capture_train_step(B, lr=LR, n_steps=3)
    sx.copy_(_batch(case, 3))
    d, ws = e._workspace(B)
    cell = ws[L.workspace_offset(d, e.model, "clip_norm") // 4:][:1]
    assert float(cell) == 1.0                           # (the engine filled it)
    cell.zero_()
    before = _state(e)
    rp()
    torch.cuda.synchronize()
    assert _same(before, _state(e)) and torch.isnan(rp.grad_clip[:, 3]).all() and int(e.step_dev[0]) == 3
    assert torch.isfinite(rp.tail_log[:, 0]).all()
    cell.fill_(1.0)
    rp()
    torch.cuda.synchronize()
    assert not _same(before, _state(e)) and torch.isfinite(rp.grad_clip).all()


# ------------------------------------------------------------------ the measurement loops
@pytest.mark.parametrize("mode", [0, 1])
def test_bench_loop_writes_record_zero_and_profiles_refuse(mode):
    """gmvae_bench_loop (eager launches / one captured graph) clips through record 0; gmvae_step_profile honours the bit,
    gmvae_train_profile refuses it."""
    import torch
    L = _L()
    case = "gmvae-small"
    B = CASES[case]["B"]
    e = _engine(case, 1e-3)                             # (far below any norm of these sizes: every step clips)
    x = _batch(case)
    d, ws = e._workspace(B)
    before = _state(e)
    usec = C.c_float()
    rc = L.lib.gmvae_bench_loop(C.byref(d), e.model, L.ptr(x), L.ptr(e.params), L.ptr(e.m), L.ptr(e.v), L.ptr(e.grads), L.ptr(ws),
                                L.ptr(e.step_dev), 2, mode, C.byref(usec), L.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and usec.value > 0
    e.global_step = int(e.step_dev[0])
    assert e.global_step == 3 + mode                    # (a first step, the graph's warm-up launch, then the two timed ones)
    rec = e._clip_records(d, ws)[0].cpu().numpy()
    clip_ref.check_record(rec, e.grads.cpu().numpy(), 1e-3)
    assert rec[2] == 1.0 and not _same(before, _state(e)) and all(torch.isfinite(t).all() for t in _state(e))
    assert [n for n, _, _ in e.profile_levels(x, iters=1)][-1] == "finalize_grads_ss"
    with pytest.raises(L.GmvaeError, match="GMVAE_E_DIMS"):
        e.profile_train_levels(x, iters=1)


# ------------------------------------------------------------------ 8. run_train
@pytest.mark.parametrize("eager", [False, True])
def test_run_train_logs_the_gradient_norm(tmp_path, capsys, eager):
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args(
        ["--mode=train", "--model=gmvae", "--latent_size=8", "--hidden_size=32", "--batch_size=16", "--max_steps=7",
         "--summarise_every=4", f"--logdir={tmp_path}", "--random_seed=3", "--synthetic_size=256", "--data_dim=64",
         "--clip_norm=0.5"] + (["--eager"] if eager else [])))
    m = runners.run_train(cfg)
    assert m._engine.global_step == 8 and m._engine.clip_norm == 0.5
    assert runners.run_train.last_path == ("eager" if eager else "pipeline-graph")
    log = runners.run_train.clip_log
    assert sum(w["steps"] for w in log) == 8 and len(log) == 2
    for w in log:
        assert math.isfinite(w["mean"]) and math.isfinite(w["max"]) and 0 < w["mean"] <= w["max"]
        assert 0.0 <= w["clipped_share"] <= 1.0 and w["skipped_share"] == 0.0
    out = capsys.readouterr().out
    assert "grad_norm mean" in out and "clipped" in out and "skipped" in out
