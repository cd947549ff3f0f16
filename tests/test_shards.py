"""The sharding contract of GmvaeDims::row0 on the device (tests/shard_cases.py has the tables, tests/test_shards_cpu.py holds them
without a device).

Part A -- shards add up, family by family: a batch of 11 rows stepped whole at row0 = 5 and as shards of 1, 6 and 4 rows at
row0 = 5, 6, 12 with in-kernel noise; the counts of the tail add exactly, the loss sum and every gradient tensor of the shard sum
meet the whole-batch device step at 2e-6 / 2e-5 (no ReLU allowance: the cases keep every unit off its kink), and both the whole
step and the shard sum meet the family's fp64 statement on the regenerated noise at the family's standing gates.  The clip and one
Adam step on the host-summed buffer; the same sums through Engine.step on sliced views of one batch tensor, for each kind of
per-example input.

Part B -- every noise site past 2^31, 2^32 and at the top of the Philox row field: the step on every leading schedule word, the
evaluators and gmvae_impute at row0 chosen so that the boundary falls inside the call, against the fp64 statement on oracle.noise
at the true rows; the chains (gmvae_ais, its reverse, gmvae_refine) and gmvae_simulate against the call on gmvae_noise_fill's noise
and that noise against oracle.noise; three train-graph corners on rank floor(2^32 / B); gmvae_binarize at a 64-bit out_row0;
Engine.aggregate_posterior's samples at row0 and at its default rank * M.  A
32-bit row anywhere misses these gates at least 10 times over (asserted without a device).  Rows one at a time at row0 + b give
the bits of the batched call -- the fused forward, the chains, simulate, impute's draws -- except on the general schedule's
evaluators, whose GEMM tilings follow the batch size: those meet at tests/test_iw_bound.py's 1e-5.

profiles/shard_notes.md records the margins of one run on an MI355X."""
import numpy as np
import pytest

import oracle as O
import shard_cases as SC
from hip_util import _L, check_grads, chunked_call, hip_step, tail_gates
from test_count import cstep
from test_dreg import dstep
from test_lik import lik_gates, lstep, sq_gates
from test_pmask import pstep
from test_realx import rstep
from test_wobj import wstep
from test_ytemp import ystep

pytestmark = pytest.mark.gpu

_RUNS = {}         # family id -> (whole, [shards]): each (grad sums [P] float64, tail [8], ReLU masks); run once, shared


def step_rows(P, a, b, row0):
    """The family's own step helper on rows a .. b - 1 of the batch at row0, in-kernel noise: (grad sums, tail, ReLU masks)."""
    f, x = P.f, P.x[a:b]
    head = (P.model, P.d, P.flat, x, None, None)
    if f.kind == "mask":
        return pstep(*head, P.extra["mask"][a:b], row0=row0)
    if f.kind == "lik":
        return lstep(*head, f.opt, f.sigma, row0=row0)
    if f.kind == "realx":
        return rstep(*head, f.flags, f.sigma, row0=row0)[:3]
    if f.kind == "count":
        return cstep(*head, f.flags, row0=row0)[:3]
    if f.kind == "weights":
        return wstep(P.model, f.opt == "marginal", P.d, P.flat, x, None, None, P.extra["weights"], row0=row0)
    if f.kind == "temp":
        return ystep("shards", SC.TAU, bool(f.flags & SC.Y_STRAIGHT_THROUGH), case=(P.d, P.p32, P.flat, x, None, None), row0=row0)[:3]
    if f.kind == "dreg":
        r = dstep(P.model, P.d, P.d.S, P.flat, x, None, f.flags, row0=row0)
        assert r["schedule"].endswith("+dreg")
        return r["g"], r["tail"], r["masks"]
    return hip_step(P.model, P.d, P.flat, x, None, None, SC.SEED, SC.STEP, want_masks=True, row0=row0)


def runs(id):
    if id not in _RUNS:
        P = SC.problem(id)
        _RUNS[id] = (step_rows(P, 0, SC.B, SC.ROW0), [step_rows(P, a, b, SC.ROW0 + a) for a, b in SC.CUTS])
    return _RUNS[id]


def add_up(shards):
    """The all-reduce on the host: gradient sums and tails added, the ReLU masks stacked by rows."""
    gs = sum(s[0] for s in shards)
    tail = sum(s[1] for s in shards)
    masks = {net: [None] + [np.concatenate([s[2][net][i] for s in shards]) for i in range(1, len(ms))]
             for net, ms in shards[0][2].items()}
    return gs, tail, masks


def tensors(P):
    """[(name, offset, size)] of every gradient tensor, the appended rho included."""
    lay, _, _ = O.param_layout(P.model, P.d)
    out = [(name, off, int(np.prod(shape))) for name, shape, off in lay]
    if SC.rho_name(P.f):
        out.append((SC.rho_name(P.f), P.flat.shape[0] - (P.d.D + 3) // 4 * 4, P.d.D))
    return out


def hold_to_statement(P, what, gs, tail, masks):
    """A3: a step's buffer (whole or summed) against the fp64 statement on the regenerated noise at the family's standing
    gates.  Returns the worst error as a fraction of its gate."""
    f, B, D = P.f, SC.B, P.d.D
    Cc, g = SC.statement(f.id)
    assert np.isfinite(gs).all() and np.isfinite(tail).all()
    if f.kind in ("lik", "realx", "count"):
        lik_gates(what, tail, B, Cc)
        sq_gates(what, tail, B, D, Cc)
        worst = [abs(tail[0] / B - Cc["loss"]) / (1e-4 * max(abs(Cc["loss"]), Cc["nll_abs"]))]
    else:
        tail_gates(what, tail, B, Cc)
        worst = [abs(tail[0] / B - Cc["loss"]) / (1e-4 * abs(Cc["loss"]))]
    if f.kind == "mask":
        assert abs(tail[5] - Cc["hid"]) <= 1e-4 * abs(Cc["hid"]), (what, tail[5], Cc["hid"])
        assert tail[6] == Cc["n_missing"] and tail[7] == Cc["n_observed"]
    if f.kind == "weights":
        w32 = np.asarray(P.extra["weights"], np.float32)
        assert tail[5] == float(np.float32(B) * w32[0]) and tail[6] == float(np.float32(B) * w32[1]), (what, tail[5:7])
        assert tail[7] == Cc["floor"].sum() and 0 < tail[7] < B, (what, tail[7], Cc["floor"])
    errs = check_grads(what, P.model, P.d, gs, g, B, masks, Cc["pre"], lambda m: P.statement(relu_masks=m)[1])
    worst += [e / 1e-4 for _, e in errs]
    rho = SC.rho_name(f)
    if rho:
        _, off, n = tensors(P)[-1]
        got, ref = gs[off:off + n] / B, g[rho]
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
        print(f"{what} {rho}: rel-to-max err {err:.3e}")
        assert err <= 1e-4, (what, rho, err)
        assert not gs[off + n:].any()
        worst.append(err / 1e-4)
    return max(worst)


# =============================================================================================================== Part A
@pytest.mark.parametrize("id", list(SC.BY_ID))
def test_shards_add_up_to_the_whole_batch(id):
    """A1 - A3 for one family."""
    P = SC.problem(id)
    (gw, tw, mw), shards = runs(id)
    gs, ts, ms = add_up(shards)
    # A1: the counts add exactly
    for i in SC.count_entries(P.f):
        assert ts[i] == tw[i], (id, i, ts[i], tw[i])
    assert tw[4] == SC.B and [s[1][4] for s in shards] == [b - a for a, b in SC.CUTS]
    # A2: the same noise rows, another summation order
    rel = abs(ts[0] - tw[0]) / abs(tw[0])
    worst = 0.0
    for name, off, n in tensors(P):
        err = np.abs(gs[off:off + n] - gw[off:off + n]).max() / max(np.abs(gw[off:off + n]).max(), 1e-30)
        worst = max(worst, err)
        assert err <= SC.GRAD_RTOL, (id, name, err)
    print(f"[shards] A2 {id}: loss sum {rel:.2e} of {SC.LOSS_RTOL:.0e}; worst gradient tensor {worst:.2e} of {SC.GRAD_RTOL:.0e}")
    assert rel <= SC.LOSS_RTOL, (id, ts[0], tw[0])
    print(f"[shards] A2 {id}: the tail's other sums, shard sum - whole: {(ts - tw)[[1, 2, 3, 5]].tolist()} of {tw[[1, 2, 3, 5]].tolist()}")
    # A3: both against the fp64 statement of the whole batch
    a = hold_to_statement(P, f"{id} whole", gw, tw, mw)
    b = hold_to_statement(P, f"{id} shard sum", gs, ts, ms)
    print(f"[shards] A3 {id}: worst error / gate: whole batch {a:.3f}, shard sum {b:.3f}")


@pytest.mark.parametrize("id", [f.id for f in SC.FAMILIES if f.control])
def test_shards_at_row0_zero_miss_the_whole_batch(id):
    """A5, the control: with every shard at row0 = 0 the shards draw rows 0 .. and the loss is measurably another one."""
    P = SC.problem(id)
    (_, tw, _), _ = runs(id)
    wrong = sum(step_rows(P, a, b, 0)[1] for a, b in SC.CUTS)
    rel = abs(wrong[0] - tw[0]) / abs(tw[0])
    print(f"[shards] A5 {id}: shards at row0 = 0 miss the whole batch's loss by {rel:.2e}")
    assert wrong[4] == tw[4] and rel > SC.CONTROL_RTOL, (id, rel)


CLIP_CASE = "nb-gmvae-d100-s3"          # the clip with the negative binomial: rho's fp64 launch pair is part of the norm


def test_clip_on_the_summed_shards():
    """A4: the three shards' buffers summed on the host (fp32, in rank order, as a ring all-reduce would), then gmvae_grad_clip
    and one adam_tf_step on the sum.  The record and the update at tests/test_clip.py's gates (clip_ref.check_record: 2 u;
    adam_ref.bounds with count := d); the record against clip_ref on the fp64 statement's whole-batch gradient at the gradients'
    own 1e-4; and against the whole-batch device step's record at 2e-5."""
    import torch
    import adam_ref
    import clip_ref
    L = _L()
    P = SC.problem(CLIP_CASE)
    (gw, tw, _), shards = runs(CLIP_CASE)
    Pn = P.flat.shape[0]
    assert Pn % 4 == 0
    whole = np.concatenate([gw, tw]).astype(np.float32)
    summed = np.zeros(Pn + L.TAIL, np.float32)
    for g, t, _ in shards:
        summed = (summed + np.concatenate([g, t]).astype(np.float32)).astype(np.float32)
    Cc, g64 = SC.statement(CLIP_CASE)
    ref = np.zeros(Pn + L.TAIL)
    for name, off, n in tensors(P):
        ref[off:off + n] = np.asarray(g64[name]).reshape(-1) * SC.B
    ref[Pn], ref[Pn + 4] = Cc["loss"] * SC.B, SC.B
    norm64 = _record64(ref, np.inf)[0]
    Cv = float(np.float32(0.5 * norm64))                                 # the sum is clipped to half its norm
    assert not clip_ref.flag_band(summed, Cv) and not clip_ref.flag_band(whole, Cv)
    n64, d64, clipped64, skip64 = _record64(ref, Cv)
    assert clipped64 and not skip64
    HP = (1e-3, 0.9, 0.999, 1e-8)

    def clip_and_step(buf):
        gd = torch.from_numpy(buf).cuda()
        cn = torch.tensor([Cv], dtype=torch.float32).cuda()
        rec = torch.full((4,), -7.0, dtype=torch.float32).cuda()
        scratch = torch.zeros(L.grad_clip_scratch_bytes(Pn) // 8, dtype=torch.float64).cuda()
        L.check(L.lib.gmvae_grad_clip(L.ptr(gd), Pn, L.ptr(cn), L.ptr(rec), L.ptr(scratch), L.current_stream()), "gmvae_grad_clip")
        pd = torch.from_numpy(P.flat.copy()).cuda()
        md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
        L.check(L.lib.adam_tf_step(L.ptr(pd), L.ptr(md), L.ptr(vd), L.ptr(gd), Pn, *HP, 1, None, 1.0, L.ptr(rec[1:2]), L.ptr(rec[3:4]),
                                   L.current_stream()), "adam_tf_step")
        torch.cuda.synchronize()
        assert np.array_equal(gd.cpu().numpy(), buf)                     # (the clip scales nothing in place: Adam divides by d)
        return rec.cpu().numpy(), [t.cpu().numpy() for t in (pd, md, vd)]

    rec_s, state_s = clip_and_step(summed)
    rec_w, _ = clip_and_step(whole)
    w_rec = clip_ref.check_record(rec_s, summed, Cv)
    clip_ref.check_record(rec_w, whole, Cv)
    assert rec_s[2] == rec_w[2] == 1.0
    zeros = np.zeros(Pn, np.float32)
    want = adam_ref.predict(P.flat, zeros, zeros, summed[:Pn], np.float64(rec_s[1]), 1, *HP)
    bnd = adam_ref.bounds(P.flat, zeros, zeros, summed[:Pn], np.float64(rec_s[1]), 1, *HP)
    w = [adam_ref.worst(state_s[i], want[j], bnd[k])[0] for i, j, k in ((0, 0, 2), (1, 1, 0), (2, 2, 1))]
    e64 = (abs(rec_s[0] - n64) / n64, abs(rec_s[1] - d64) / d64)
    ew = (abs(rec_s[0] - rec_w[0]) / rec_w[0], abs(rec_s[1] - rec_w[1]) / rec_w[1])
    print(f"[shards] A4 {CLIP_CASE}: record of the sum {w_rec:.3f} of 2 u; p' {w[0]:.3f} m' {w[1]:.3f} v' {w[2]:.3f} of adam_ref.bounds; "
          f"norm, d against the fp64 gradient {e64[0]:.2e}, {e64[1]:.2e} of 1e-4; against the whole-batch record {ew[0]:.2e}, {ew[1]:.2e} "
          f"of {SC.GRAD_RTOL:.0e}")
    assert max(w) <= 1.0, w
    assert max(e64) <= 1e-4 and max(ew) <= SC.GRAD_RTOL


def _record64(buf64, Cv):
    """clip_ref.record's formulas on an fp64 buffer as it stands (clip_ref.record reads its buffer as the fp32 values it holds)."""
    Pn = buf64.shape[0] - 8
    root, count = float(np.sqrt(np.sum(buf64[:Pn] ** 2))), buf64[Pn + 4]
    over = root / float(np.float32(Cv))
    return root / count, max(over, count), over > count, not np.isfinite(root)


ENGINES = {     # one per kind of per-example input: constructor arguments, the step's argument
    "mask": (dict(model="gmvae", pixel_mask=True), "mask"),
    "labels": (dict(model="gmvae", y_inference="marginal", semi_supervised=True), "y_observed"),
    "f32": (dict(model="gmvae", likelihood="gaussian", likelihood_sigma=0.25, real_valued=True), None),
}


@pytest.mark.parametrize("kind", list(ENGINES))
def test_engine_steps_on_sliced_views_add_up(kind):
    """Engine.step(row0=) on x[a:b] of one contiguous [11, 13] batch tensor (the slices' bases fall off every 16-byte multiple)
    and on the matching slices of the per-example input: the three buffers sum to the whole-batch step at A2's numbers."""
    import torch
    from gmvae_amd.engine import Engine
    kw, arg = ENGINES[kind]
    D, Lz, K = 13, 4, 3
    e = Engine(kw["model"], D, Lz, K, [16], random_seed=3, **{k: v for k, v in kw.items() if k != "model"})
    e.rank = 3                                  # as on rank 3 of a larger world: row0 is passed, never rank * B
    rng = np.random.default_rng(4)
    if kind == "f32":
        x = torch.from_numpy(rng.standard_normal((SC.B, D)).astype(np.float32)).cuda()
    else:
        x = torch.from_numpy((rng.random((SC.B, D)) < 0.6).astype(np.uint8)).cuda()
    side = None
    if kind == "mask":
        side = torch.from_numpy((rng.random((SC.B, D)) < 0.7).astype(np.uint8)).cuda()
    if kind == "labels":
        side = torch.tensor([0, -1, 2, -1, 1, 1, -1, 0, 2, -1, 0], dtype=torch.int32).cuda()

    def step(a, b):
        args = {arg: side[a:b]} if arg else {}
        assert x[a:b].data_ptr() % 16 or a == 0
        buf = e.step(x[a:b], row0=SC.ROW0 + a, **args).detach().clone()
        torch.cuda.synchronize()
        return buf.cpu().numpy().astype(np.float64)

    whole = step(0, SC.B)
    acc = sum(step(a, b) for a, b in SC.CUTS)
    P = e.P
    assert np.isfinite(whole).all() and acc[P + 4] == whole[P + 4] == SC.B
    rel = abs(acc[P] - whole[P]) / abs(whole[P])
    worst = 0.0
    for name, (off, n) in _engine_tensors(e).items():
        err = np.abs(acc[off:off + n] - whole[off:off + n]).max() / max(np.abs(whole[off:off + n]).max(), 1e-30)
        worst = max(worst, err)
        assert err <= SC.GRAD_RTOL, (kind, name, err)
    print(f"[shards] engine {kind}: loss sum {rel:.2e} of {SC.LOSS_RTOL:.0e}; worst gradient tensor {worst:.2e} of {SC.GRAD_RTOL:.0e}")
    assert rel <= SC.LOSS_RTOL
    if kind in ("mask", "labels"):
        assert acc[P + 6] == whole[P + 6] and acc[P + 7] == whole[P + 7]
    wrong = sum(e.step(x[a:b], row0=0, **({arg: side[a:b]} if arg else {})).detach().clone().cpu().numpy().astype(np.float64)
                for a, b in SC.CUTS)
    assert abs(wrong[P] - whole[P]) > SC.CONTROL_RTOL * abs(whole[P])


def _engine_tensors(e):
    L = _L()
    d = e.dims(SC.B)
    return {name: (off, int(np.prod(shape))) for name, shape, off in L.param_layout(d, e.model)}


# =============================================================================================================== Part B
STEP_IDS = [e.id for e in SC.HIGH_ROWS if e.site == "step"]
CHAIN_SITES = ("ais", "ais_reverse", "refine", "simulate")
EVAL_IDS = [e.id for e in SC.HIGH_ROWS if e.site not in ("step", "impute", "aggregate_posterior") + CHAIN_SITES]
CHAIN_IDS = [e.id for e in SC.HIGH_ROWS if e.site in CHAIN_SITES]
IMPUTE_IDS = [e.id for e in SC.HIGH_ROWS if e.site == "impute"]


@pytest.mark.parametrize("id", STEP_IDS)
def test_step_draws_the_64_bit_row(id, monkeypatch):
    """gmvae_step with eps = u = NULL at a row0 whose batch straddles the boundary, against compare_step's statement on
    oracle.noise at the true rows."""
    L = _L()
    e = SC.HIGH_BY_ID[id]
    for k, v in e.env:
        monkeypatch.setenv(k, v)
    model, d, flat, p32, x = SC.step_setup(e)
    cd = L.make_dims(e.B, d.D, d.L, d.K, d.hidden, S=d.S, sched_flags=e.flags)
    word = SC.GC.BY_ID[e.case].sched if e.case in SC.GC.BY_ID else "general"
    assert L.step_schedule(cd, model).split("+")[0] == word, (id, L.step_schedule(cd, model))
    gs, tail, masks = hip_step(model, d, flat, x, None, None, e.seed, e.step, want_masks=True, flags=e.flags, row0=e.row0,
                               mask_rows=e.per)
    Cc, g = SC.step_reference(e)
    tail_gates(id, tail, e.B, Cc)
    check_grads(id, model, d, gs, g, e.B, masks, Cc["pre"], lambda m: SC.step_reference(e, relu_masks=m)[1])
    lay, _, _ = O.param_layout(model, d)
    got = ({k: tail[i] / e.B for i, k in enumerate(("loss", "nll", "kl", "nent"))},
           {name: gs[off:off + int(np.prod(shape))].reshape(shape) / e.B for name, shape, off in lay})
    print(f"[shards] B {id}: worst error / gate {SC.margin_step(e, got, (Cc, g)):.3f} (before any ReLU allowance)")
    if e.boundary == "last":                                              # (row0 + B) S [K] < 2^38: the next row0 is refused
        with pytest.raises(L.GmvaeError, match="GMVAE_E_DIMS"):
            hip_step(model, d, flat, x, None, None, e.seed, e.step, flags=e.flags, row0=e.row0 + 1)


def _evaluate(e, row0=None, rows=slice(None)):
    model, d, flat, x = SC.eval_setup(e)
    return chunked_call(e.site, model, d, flat, x[rows], e.n, SC.EVAL_CHUNK, e.row0 if row0 is None else row0, seed=e.seed,
                        step=e.step)


@pytest.mark.parametrize("id", EVAL_IDS)
def test_evaluator_draws_the_64_bit_row(id, monkeypatch):
    """n = 7 in chunks of 3 at a row0 where one example's samples straddle the boundary, against the fp64 statement of the
    evaluator's own test file at the true rows, at that file's gates."""
    L = _L()
    e = SC.HIGH_BY_ID[id]
    for k, v in e.env:
        monkeypatch.setenv(k, v)
    o = _evaluate(e)
    assert all(np.isfinite(v).all() for v in o.values()) and o["tail"][4] == e.B
    m = SC.margin_eval(e, o, SC.eval_reference(e))
    print(f"[shards] B {id}: worst error / gate {m:.3f}")
    assert m <= 1.0, (id, m)
    if e.case.startswith("iw_bound-evalf"):        # the fused forward ran: GMVAE_NO_EVALF=1 gives other bits (tests/test_iw_bound.py)
        monkeypatch.setenv("GMVAE_NO_EVALF", "1")
        g = _evaluate(e)
        assert not np.array_equal(g["bound"], o["bound"]) and SC.margin_eval(e, g, SC.eval_reference(e)) <= 1.0
        monkeypatch.delenv("GMVAE_NO_EVALF")
    if e.boundary == "last":                       # (row0 + B) n [K] < 2^38: the next row0 is refused, on real buffers
        with pytest.raises(L.GmvaeError, match=f"gmvae_{e.site}"):
            _evaluate(e, row0=e.row0 + 1)


@pytest.mark.parametrize("id", [i for i in EVAL_IDS if i.endswith("2^32")])
def test_rows_one_at_a_time_give_the_bits_of_the_batch(id, monkeypatch):
    """"The result does not depend on the chunk, the batch size or the sharding": the call on B rows against the same rows run
    one at a time at row0 + b.  Bit for bit where a row's arithmetic does not depend on the launch's other rows -- the fused
    forward (tests/test_iw_bound.py) --; the general schedule's GEMM tilings, and so their fp32 summation order, follow the
    batch size: its rows meet at that file's standing number for this comparison, 1e-5 relative (test_iw_bound.py:116) -- log_post,
    a difference of two log_joint, at 1e-5 of the row's largest |log_joint|, the scale margin_eval gates it on.  A wrong row
    moves these outputs by 10 gates of 1e-4 and more (tests/test_shards_cpu.py)."""
    e = SC.HIGH_BY_ID[id]
    for k, v in e.env:
        monkeypatch.setenv(k, v)
    whole = _evaluate(e)
    ones = [_evaluate(e, row0=e.row0 + b, rows=slice(b, b + 1)) for b in range(e.B)]
    for k in whole:
        if k == "tail":
            continue
        one = np.concatenate([o[k] for o in ones])
        if e.case.startswith("iw_bound-evalf"):
            assert np.array_equal(one, whole[k]), (id, k)
        elif k == "log_post":
            assert np.all(np.abs(one - whole[k]) <= 1e-5 * np.abs(whole["log_joint"]).max(axis=1, keepdims=True)), (id, k)
        else:
            assert np.allclose(one, whole[k], rtol=1e-5, atol=0), (id, k, one, whole[k])


@pytest.mark.parametrize("id", IMPUTE_IDS)
def test_impute_draws_the_64_bit_row(id):
    """gmvae_impute (its own Philox row in impute_merge's draws, the evaluators' in its samples): the log weights at
    tests/test_impute.py's row gate and the resampled indices wherever the statement's two best keys can be told apart."""
    import impute_cases as IC
    import impute_ref as IR
    from test_impute import impute
    L = _L()
    e = SC.HIGH_BY_ID[id]
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(e.case)
    assert (e.seed, e.step) == (IC.SEED, IC.STEP) and xf.shape[0] == e.B
    o = impute(model, d, flat, xf, m, e.n, SC.EVAL_CHUNK, row0=e.row0)
    s, est = SC.impute_reference(e)
    mg = SC.margin_impute(o["logw"], s["lw"])
    print(f"[shards] B {id}: worst log-weight error / gate {mg:.3f}")
    assert mg <= 1.0
    cmpd = IR.compared_draws(s["lw"], est["key_gap"])
    assert 1.0 - cmpd.mean() <= IC.MAX_LEFT_OUT
    assert np.array_equal(o["draw_index"][cmpd], est["draw_index"][cmpd])
    wrong = SC.impute_reference(e, wrong=True)[1]["draw_index"]
    assert not np.array_equal(wrong[cmpd], est["draw_index"][cmpd])          # (the draws tell a 32-bit row apart too)
    if e.boundary == "last":
        with pytest.raises(L.GmvaeError, match="gmvae_impute"):
            impute(model, d, flat, xf, m, e.n, SC.EVAL_CHUNK, row0=e.row0 + 1)
    if e.boundary == "2^32":                       # the rows one at a time at row0 + b, as tests/test_impute.py does at row0 = b
        from test_impute import _within_weight_bound
        rows = [impute(model, d, flat, xf[b:b + 1], m[b:b + 1], e.n, SC.EVAL_CHUNK, row0=e.row0 + b) for b in range(e.B)]
        one = {k: np.concatenate([r[k] for r in rows]) for k in ("mean", "stats", "logw", "draw_index", "draw_z")}
        _within_weight_bound(o, one, f"{id}: B = {e.B} against one row at a time")
        assert np.array_equal(o["draw_index"], one["draw_index"])


def _bits_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("id", CHAIN_IDS)
def test_chain_sites_draw_the_64_bit_row(id):
    """gmvae_ais, gmvae_ais_reverse (Philox row (row0 + b) n_chains + c), gmvae_refine ((row0 + b) S + s) and gmvae_simulate
    (row0 + b) at rows that straddle the boundary.  Their own test files state them on the noise gmvae_noise_fill gives at the
    same rows, so: the call on its in-kernel noise gives the bits of the call on that noise supplied as arrays (at row0 = 0: the
    arrays alone key it), and that noise is oracle.noise at the true rows -- the uniforms bit for bit, the normals at
    tests/test_hip_parity.py's 2e-5."""
    import torch
    import ais_ref as AR
    import bdmc_cases as BK
    from test_ais import device_ais, device_noise
    from test_bdmc import device_rev, device_sim, device_sim_noise
    L = _L()
    e = SC.HIGH_BY_ID[id]
    model, d = SC.chain_dims()
    p, flat = BK.make(model, d, 2000)
    ref = SC.chain_noise(e)
    if e.site == "simulate":
        def call(row0, *noise, b=None):
            return device_sim(model, d, flat, e.B if b is None else 1, *noise, row0=row0, seed=e.seed, step=e.step)
        noise = device_sim_noise(e.B, d, e.row0, e.seed, e.step)
    elif e.site == "refine":
        import refine_ref as RF
        from test_refine import device_noise as refine_noise, device_refine
        pr, flat, x_all = RF.make(model, d, e.B, 77)
        start_all = RF.start_table(model, d, pr, x_all).astype(np.float32)

        def call(row0, *noise, b=None):
            x, start = (x_all, start_all) if b is None else (x_all[b:b + 1], start_all[b:b + 1])
            return device_refine(model, d, flat, x, start, SC.REFINE_STEPS, SC.REFINE_S, SC.REFINE_ROUNDS, *noise, row0=row0,
                                 seed=e.seed, step=e.step)
        noise = (refine_noise(SC.REFINE_STEPS + SC.REFINE_ROUNDS, e.B * SC.REFINE_S, d.L, e.row0 * SC.REFINE_S, e.seed, e.step),)
    else:
        x_all = (np.random.default_rng(5).random((e.B, d.D)) < 0.5).astype(np.uint8)
        betas = AR.schedule("sigmoid", SC.CHAIN_T).astype(np.float32)
        z_all = np.random.default_rng(6).standard_normal((e.B, d.L)).astype(np.float32)

        def call(row0, *noise, b=None):
            eps, u = noise if noise else (None, None)
            x, z0 = (x_all, z_all) if b is None else (x_all[b:b + 1], z_all[b:b + 1])
            if e.site == "ais":
                return device_ais(model, d, flat, x, betas, SC.CHAIN_C, SC.CHAIN_LEAP, 0.5, None, eps, u, row0=row0, seed=e.seed,
                                  step=e.step)
            return device_rev(model, d, flat, x, z0, betas, SC.CHAIN_C, SC.CHAIN_LEAP, 0.5, None, eps, u, row0=row0, seed=e.seed,
                              step=e.step)
        noise = device_noise(SC.CHAIN_T, e.B * SC.CHAIN_C, d.L, e.row0 * SC.CHAIN_C, e.seed, e.step)
    own = call(e.row0)
    assert all(np.isfinite(v).all() for k, v in own.items() if v.dtype.kind == "f")
    _bits_equal(own, call(0, *noise))
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in noise]
    if e.site in ("ais", "ais_reverse"):        # (slot 0 of the chains' uniforms is not drawn from: tests/bdmc_cases.py)
        got[1], ref = got[1][1:], (ref[0], ref[1][1:])
    assert all(np.array_equal(g, r) for g, r in zip(got[1:], ref[1:]))
    m = SC.margin_noise(got[:1], ref[:1])
    print(f"[shards] B {id}: in-kernel noise = supplied noise, bit for bit; normals against oracle.noise {m:.3f} of {SC.NOISE_ATOL:.0e}")
    assert m <= 1.0
    if e.boundary == "last":
        with pytest.raises(L.GmvaeError, match="GMVAE_E_DIMS"):
            call(e.row0 + 1)
    if e.boundary == "2^32":                       # the examples one at a time at row0 + b: the bits of the batched call, as the
        ones = [call(e.row0 + b, b=b) for b in range(e.B)]              # sites' own files hold for halves at row0 = 0, 2
        for k in own:
            if k != "tail":
                one = np.concatenate([o[k] for o in ones], axis=1 if k == "trace" else 0)
                assert np.array_equal(one.view(np.uint8), own[k].view(np.uint8)), (id, k)


# the train graphs' schedules read step_dev and form their Philox row in mega2_body / mega2v_body / mega_fwd_bwd with the first layer
# inside the launch.  (corner of tests/gate_corners.py: the smallest `train` corner of each schedule whose batch can straddle 2^32
# at row0 = rank * B -- a batch of one row cannot.)
@pytest.mark.parametrize("cid", SC.TRAIN_CORNERS)
def test_train_graph_draws_the_64_bit_row(cid):
    """Three steps of a train graph on rank = floor(2^32 / B) of a larger world: rows rank B .. rank B + B - 1 straddle 2^32.
    Against three fp64 steps on the noise of those rows at tests/test_timed_path.py's gates (the last step's loss terms and
    gradients, the parameters inside their Adam-derived tolerance); tests/test_shards_cpu.py shows that the first step on the rows
    a 32-bit row would give misses those gates."""
    import torch
    import test_timed_path as T
    from gmvae_amd.engine import Engine
    L = _L()
    c = SC.GC.BY_ID[cid]
    d, B, n = c.d, c.B, 3
    rank = SC.TWO32 // B
    assert rank * B < SC.TWO32 < rank * B + B - 1
    mid = O.MODEL_NAMES[c.model]
    e = Engine(c.model, d.D, d.L, d.K, list(d.hidden), random_seed=4)
    e.rank = rank
    assert e.dims(B).row0 == rank * B and L.step_schedule(e.dims(B), e.model).split("+")[0] == c.sched
    flat0 = e.params.detach().cpu().numpy()
    xs = (np.random.default_rng(B).random((n, B, d.D)) < 0.87).astype(np.uint8)
    sx, replay = e.capture_train_step(B, lr=T.LR, n_steps=n)
    sx.copy_(torch.from_numpy(xs).cuda())
    replay()
    torch.cuda.synchronize()
    assert e.handoff_timeouts() == 0 and e.global_step == n and int(e.step_dev[0].item()) == n
    # as test_timed_path.trajectory_case: a second engine on the same rank steps a ONE-step graph n times (the same bits) and hands
    # the oracle the device's ReLU masks and its parameters before every step
    e1 = Engine(c.model, d.D, d.L, d.K, list(d.hidden), random_seed=4)
    e1.rank = rank
    sx1, replay1 = e1.capture_train_step(B, lr=T.LR, n_steps=1)
    masks, pre = [], []
    xd = torch.from_numpy(xs).cuda()
    for t in range(n):
        pre.append(e1.params.detach().cpu().numpy().astype(np.float64))
        sx1.copy_(xd[t])
        replay1()
        torch.cuda.synchronize()
        masks.append(T._device_masks(e1, mid, d, B))
    assert torch.equal(e1.params, e.params)
    flat_ref, Cc, g, gs = T._oracle_trajectory(L, mid, d, flat0, xs, e.noise_seed, row_base=rank * B, masks_of_step=lambda t: masks[t],
                                               params_of_step=lambda t: pre[t], tag=cid)
    eps, u = T._noise(L, B * d.S, d.L, d.K, rank * B, e.noise_seed, n - 1, mid == O.MODEL_GMVAE)
    ref_eps, ref_u = O.noise(B * d.S, d.L, d.K, rank * B, e.noise_seed, n - 1)      # (the trajectory's noise is gmvae_noise_fill's)
    assert np.abs(eps - ref_eps).max() <= SC.NOISE_ATOL and (u is None or np.array_equal(u, ref_u))
    C2, g2 = O.loss_and_grads(mid, d, O.unpack(mid, d, pre[n - 1]), xs[n - 1], eps, u, np.float64, relu_masks=masks[n - 1])
    T._compare_last_step(mid, d, e, B, Cc, g, at_device=(C2, O.pack(mid, d, g2, np.float64)), tag=cid)
    T._compare_params(mid, d, e, flat_ref, gs, n, cid)


@pytest.mark.parametrize("name,out_row0", SC.BINARIZE)
def test_binarize_draws_the_64_bit_position(name, out_row0):
    """gmvae_binarize with out_row0 so that the global quad index crosses 2^31 / 2^32 inside the batch, or ends at 2^62 - 1:
    oracle.binarize's pixels bit for bit, and the rows one at a time at out_row0 + b give the same."""
    import torch
    L = _L()
    pix, ref = SC.binarize_case(out_row0)
    pd = torch.from_numpy(pix).cuda()

    def call(rows, at):
        x = torch.full((len(rows), SC.BIN_D), 255, dtype=torch.uint8, device="cuda")
        L.check(L.lib.gmvae_binarize(L.ptr(pd), SC.BIN_B, None, rows[0], len(rows), SC.BIN_D, 11, 3, None, L.ptr(x), at,
                                     L.current_stream()), "gmvae_binarize")
        torch.cuda.synchronize()
        return x.cpu().numpy()

    got = call(range(SC.BIN_B), out_row0)
    assert np.array_equal(got, ref), (name, int((got != ref).sum()))
    ones = np.concatenate([call([b], out_row0 + b) for b in range(SC.BIN_B)])
    assert np.array_equal(ones, ref)


AGG_IDS = [e.id for e in SC.HIGH_ROWS if e.site == "aggregate_posterior"]


@pytest.mark.parametrize("id", AGG_IDS)
def test_aggregate_posterior_samples_the_64_bit_row(id):
    """Engine.aggregate_posterior's own path to the noise -- row0 (and its default rank * M) as a Python int through ctypes, keyed
    by (noise_seed, global_step): 7 queries whose rows row0 + m straddle the boundary, z against tests/aggpost_ref.py's sample on
    oracle.noise at the true rows, at tests/test_aggpost.py's gate."""
    import torch
    import aggpost_ref as AG
    from gmvae_amd.engine import Engine
    e = SC.HIGH_BY_ID[id]
    mname, d, model, p, flat, x = SC.aggpost_case()
    eng = Engine(mname, d.D, d.L, d.K, list(d.hidden), sigma_min=d.sigma_min, raw_sigma_bias=d.raw_sigma_bias, random_seed=1)
    with torch.no_grad():
        eng.params.copy_(torch.from_numpy(flat[:eng.P]))
    eng.noise_seed, eng.global_step = e.seed, e.step
    xd, q = torch.from_numpy(x).cuda(), torch.from_numpy(SC.AGG_QUERIES)
    got = eng.aggregate_posterior(xd, queries=q, row0=e.row0)
    z_ref, k_ref = SC.aggpost_reference(e)
    m = SC.margin_aggpost(got["z"].cpu().numpy(), z_ref)
    print(f"[shards] B {id}: worst |z - ref| / gate {m:.3f}; components drawn {np.bincount(k_ref, minlength=d.K).tolist()}")
    assert m <= 1.0 and all(bool(torch.isfinite(got[k]).all()) for k in ("log_q_zx", "log_q_z", "log_p_z"))
    if e.row0 % e.B == 0:                         # the 2^32 entry sits at rank * M: the default row0 of rank floor(2^32 / M) draws the same
        eng.rank = e.row0 // e.B
        assert torch.equal(eng.aggregate_posterior(xd, queries=q)["z"], got["z"])
