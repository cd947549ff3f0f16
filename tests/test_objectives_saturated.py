"""-m gpu: the objective variants' training steps OUTSIDE the Xavier regime, against the fp64 statement of their path.

tests/test_saturated.py runs every fast path where a trained or a diverging model lives; the per-example kernels of the
`general+...` schedules -- ymarg_rows / ymarg_iw_rows (csrc/ymarg.hpp), ymarg_sup_rows / sup_tail (csrc/semisup.hpp), wobj_rows /
ymarg_wobj_rows / y_head_bwd_w / wobj_tail (csrc/wobj.hpp), z_head_bwd_dreg (csrc/kernels.hpp) -- met only Xavier parameters:
q(y|x) near uniform, importance weights of one order.  Here one gmvae_step through the C ABI on explicit noise runs at the cases
of tests/saturated_cases.py (two regimes, `trained` and `diverging`; q(y|x) one-hot with entries that are 0 in fp32, a labelled
example whose q_bc is 0 in fp32, sample groups collapsed onto one sample, examples on both sides of the free-bits floor, on it,
and none with lambda = 0), whose conditions tests/test_objectives_saturated_cpu.py asserts on the fp64 statements alone.

The drivers and the gates are the paths' own (tests/test_ymarg.py, test_semisup.py, test_dreg.py, test_wobj.py: loss 1e-4
relative, nll / kl / nent each relative to itself or to 1, every gradient tensor at 1e-4 of its own max, check_masks and a
restatement under the device's ReLU masks, tail[5..7] exact); on top, every value of the gradient buffer and the tail is finite
and the schedule string names the path.  Then the forward-only consumers of the same terms -- gmvae_iw_bound_enum_y,
gmvae_posterior_y, gmvae_posterior_component -- at the tolerances of their own files."""
import numpy as np
import pytest

import oracle as O
import saturated_cases as SC

pytestmark = pytest.mark.gpu


def _L():
    from gmvae_amd import _lib
    return _lib


def _flips():
    import hip_util
    return len(hip_util.FLIPS)


def _finite(name, gs, tail, flips0):
    print(f"{name}: ReLU units restated under the device's masks: {_flips() - flips0}")
    assert np.isfinite(tail).all(), (name, tail)
    bad = np.flatnonzero(~np.isfinite(gs))
    assert bad.size == 0, (name, bad.size, bad[:8], gs[bad[:8]])


# 1 ---------------------------------------------------------------------------------------------- y summed out, S = 1
@pytest.mark.parametrize("name", SC.names("marginal"))
def test_marginal_step(name):
    import test_ymarg as TY
    L = _L()
    c, i, f0 = SC.CASES[name], SC.inputs(name), _flips()
    sched = L.step_schedule(TY._mdims(c.d, c.B), O.MODEL_GMVAE)
    assert sched == "general+marginal", sched                      # (the one-launch sizes included: general here)
    gs, tail, Cc = TY.compare_step(c.d, i["flat"], i["x"], i["eps"], name, ref=SC.statement(name))
    _finite(name, gs, tail, f0)
    assert not tail[5:].any()


# 2 ------------------------------------------------------------- S importance samples, observed labels, DReG on top
@pytest.mark.parametrize("name", SC.names("marginal_iw") + SC.names("labels"))
def test_importance_weighted_and_labelled_step(name):
    import test_semisup as TS
    L = _L()
    c, i, f0 = SC.CASES[name], SC.inputs(name), _flips()
    flags = L.OBJ_MARGINAL_Y_IW | (L.OBJ_LABELS if c.labels else 0) | (L.GRAD_DREG if c.dreg else 0)
    sched = L.step_schedule(TS._sdims(c.d, c.B, c.S, flags=flags), O.MODEL_GMVAE)
    assert sched == "general+marginal_iw" + ("+labels" if c.labels else "") + ("+dreg" if c.dreg else ""), sched
    y = SC.labels_of(name)
    gs, tail, Cc = TS.compare_step(c.d, c.S, i["flat"], i["x"], i["eps"], y, SC.ALPHA, name, flags=flags,
                                   estimator="dreg" if c.dreg else "standard", ref=SC.statement(name))
    _finite(name, gs, tail, f0)
    if c.labels == "argmax":
        assert tail[6] == tail[7] == c.B
    elif c.labels == "argmin":
        assert tail[6] == c.B and tail[7] == 0
    elif c.labels is None:
        assert not tail[5:].any()


# 3 ------------------------------------------------------------------------------------- DReG for the VAE family
@pytest.mark.parametrize("name", SC.names("dreg"))
def test_dreg_step_of_the_vae_family(name):
    import test_dreg as TD
    L = _L()
    c, i, f0 = SC.CASES[name], SC.inputs(name), _flips()
    got = TD.dstep(i["model"], c.d, c.S, i["flat"], i["x"], i["eps"], L.GRAD_DREG)
    assert got["schedule"] == "general+dreg", got["schedule"]
    TD.check_step(name, dict(model=i["model"], d=c.d, B=c.B, S=c.S, flat=i["flat"], x=i["x"], eps=i["eps"], dreg=got),
                  ref=SC.statement(name))
    _finite(name, got["g"], got["tail"], f0)


# 4 ------------------------------------------------------------------------------------- the weighted objective
@pytest.mark.parametrize("name", SC.names("weights"))
def test_weighted_step(name):
    import test_wobj as TW
    L = _L()
    c, i, f0 = SC.CASES[name], SC.inputs(name), _flips()
    model = i["model"]
    marginal = model == O.MODEL_GMVAE and not c.gumbel
    sched = L.step_schedule(TW._cdims(model, marginal, c.d, c.B), model)
    assert sched == ("general+marginal+weights" if marginal else "general+weights"), sched
    weights = SC.weights_of(name)
    Cc, _ = SC.statement(name)
    gs, tail = TW.compare_step(name, weights, name, case=(model, marginal, c.d, i["p32"], i["flat"], i["x"], i["eps"], i["u"]),
                               ref=SC.statement(name))
    _finite(name, gs, tail, f0)
    if model == O.MODEL_GMVAE:
        want = {"all_floor": c.B, "none": 0}.get(c.lam)
        assert want is None or tail[7] == want, (name, tail[7])
        assert c.lam != "split" or 0 < tail[7] < c.B
    if c.gumbel and c.d.K > 1:                                      # the uniform stream's extremes are where the case put them
        assert i["u"][0, 0] == np.float32(O.TINY_F32) and i["u"][1, c.d.K - 1] == np.float32(SC.U_MAX)


# 5 --------------------------------------------------------------------- the forward-only consumers of the same terms
def test_enumerated_bound_and_posterior_over_y():
    from test_iw_enum import enum, fp64_bound
    from test_posterior_y import _check_self_consistent, ess_of, forward, fp64_log_w, log_softmax, lse, post
    name = "forward-h24x2-trained"
    c, i = SC.FORWARD[name], SC.inputs(name)
    d, B, n, flat, x = c.d, c.B, SC.FORWARD_N, i["flat"], i["x"]
    q = SC.q_of(name)
    assert (q < 1e-38).any()                                        # entries of q(y|x) that are 0 in fp32
    ref, ref_mlw = fp64_bound(name, d, flat, x, n)
    lw = fp64_log_w(name, d, flat, x, n)                            # [B, n, K]
    ref_lj = lse(lw, axis=1) - np.log(n)
    ref_lp = log_softmax(ref_lj)
    ref_ess = np.array([ess_of(lw[b]) for b in range(B)])
    delta = 1e-4 * np.abs(lw).reshape(B, -1).max(1)
    _, _, logits = forward(d, flat, x, 1, _L().OBJ_MARGINAL_Y)       # the schedule the chunks run: the same logits
    for chunk in (SC.FORWARD_CHUNK, n):
        bound, mlw, tail = enum(d, flat, x, n, chunk)
        print(name, chunk, "bound rel", (np.abs(bound - ref) / np.abs(ref)).max(), "mean log w rel", (np.abs(mlw - ref_mlw) / np.abs(ref_mlw)).max())
        assert np.isfinite(bound).all() and np.isfinite(mlw).all() and np.isfinite(tail).all()
        assert np.all(np.abs(bound - ref) <= 1e-4 * np.abs(ref)), (chunk, bound, ref)
        assert np.all(np.abs(mlw - ref_mlw) <= 1e-4 * np.abs(ref_mlw)), (chunk, mlw, ref_mlw)
        assert np.all(mlw <= bound)
        assert tail[4] == B and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * abs(tail[0])
        o = post(d, flat, x, n, chunk)
        assert all(np.isfinite(v).all() for v in o.values()), {k: v for k, v in o.items() if not np.isfinite(v).all()}
        lj, lp, ess = o["log_joint"].astype(np.float64), o["log_post"].astype(np.float64), o["stats"][:, 3].astype(np.float64)
        print(name, chunk, "log_joint rel", (np.abs(lj - ref_lj) / np.abs(ref_lj)).max(), "log_post abs", np.abs(lp - ref_lp).max(),
              "ess ratio", (ess / ref_ess).min(), (ess / ref_ess).max())
        assert np.all(np.abs(lj - ref_lj) <= 1e-4 * np.abs(ref_lj)), (chunk, lj, ref_lj)
        assert np.all(np.abs(lp - ref_lp) <= 2e-4 * np.abs(ref_lj).max(1, keepdims=True)), (chunk, lp, ref_lp)
        assert np.all(np.abs(np.log(ess / ref_ess)) <= 4 * delta), (chunk, ess, ref_ess)
        assert np.all(ess >= 1) and np.all(ess <= n * d.K)
        assert np.all(np.abs(np.exp(lp).sum(1) - 1.0) <= 1e-6)
        _check_self_consistent(o, logits, B, d.K)                    # bound, H(r), KL(q || r) with q_bk = 0 in fp32, the sums


def test_posterior_over_the_mixture_component():
    import post_comp_ref as R
    from test_posterior_component import SEED, STEP, _check_fp64, post
    name = "forward-vae_gmp-trained"
    c, i = SC.FORWARD[name], SC.inputs(name)
    n = SC.FORWARD_N
    lw = R.log_w(c.d, i["flat"], i["x"], n, 0, SEED, STEP)
    assert np.isfinite(lw).all()
    for chunk in (SC.FORWARD_CHUNK, n):
        o = post(c.d, i["flat"], i["x"], n, chunk)
        _check_fp64(name, o, lw, n, chunk)
        assert np.all(np.abs(np.exp(o["log_post"].astype(np.float64)).sum(1) - 1.0) <= 1e-6)
