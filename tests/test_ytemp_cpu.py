"""The device-side Gumbel-softmax temperature and the straight-through y (GMVAE_Y_TEMP_DEV, GMVAE_Y_STRAIGHT_THROUGH) without a
device: the fp64 statement (tests/ytemp_ref.py) against the oracle and a hand-applied softmax Jacobian, the library's flags /
workspace / refusals / schedule names, the Python argument checks, the annealing schedule and the CLI."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import oracle as O
import wobj_ref as WR
import ytemp_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_DIMS, E_MODEL, E_NET = -2, -3, -5          # include/gmvae_hip.h GMVAE_E_*


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def r256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("name", list(TR.CASES))
def test_relaxed_statement_is_the_existing_objective(name):
    """Relaxed y at tau = the dims' temperature: the oracle's ELBO (any S), wobj_ref's weighted one under weights."""
    d, p, flat, x, eps, u = TR.setup(name)
    w = TR.case_weights(name)
    import dataclasses
    d7 = dataclasses.replace(d, temperature=0.7)
    Ct, gt = TR.loss_and_grads(d, p, x, eps, u, 0.7, weights=w)
    if w is None:
        Cr, gr = O.loss_and_grads(O.MODEL_GMVAE, d7, p, x, eps, u, np.float64)
    else:
        Cr, gr = WR.loss_and_grads(O.MODEL_GMVAE, d7, p, x, eps, u, w)
    for k in ("loss", "nll", "kl", "nent"):
        assert abs(Ct[k] - Cr[k]) <= 1e-12 * max(abs(Cr[k]), 1.0), k
    for k in gr:
        assert np.abs(gt[k] - gr[k]).max() <= 1e-11 * max(np.abs(gr[k]).max(), 1.0), k


@pytest.mark.parametrize("name", list(TR.CASES))
@pytest.mark.parametrize("tau", TR.TAUS + (0.1,))
def test_straight_through_dlogits_is_the_softmax_jacobian_at_y_hard(name, tau):
    """Known answer: dL/dy taken at a LEAF y_hard, pulled through the relaxed sample by hand in NumPy -- da = y_soft (dy -
    sum_k y_soft dy), dlogits_b = sum_s da / tau + the entropy term's gradient -- is the straight-through statement's dlogits;
    its y rows are exact one-hot at the argmax of logits + g, and forward values do not depend on tau."""
    d, p, flat, x, eps, u = TR.setup(name)
    w = TR.case_weights(name)
    B, S, K = x.shape[0], d.S, d.K
    Cs, gs = TR.loss_and_grads(d, p, x, eps, u, tau, straight_through=True, weights=w)
    Cl, gl = TR.loss_and_grads(d, p, x, eps, u, tau, weights=w, y_leaf=True)
    assert Cs["loss"] == Cl["loss"] and np.array_equal(Cs["y"], Cl["y"])
    assert ((Cs["y"] == 0) | (Cs["y"] == 1)).all() and (Cs["y"].sum(axis=1) == 1).all()
    assert np.array_equal(Cs["y"].argmax(axis=1), Cs["argmax"])
    g64 = -np.log(-np.log(np.asarray(u, np.float64).reshape(B * S, K)))
    assert np.array_equal((np.repeat(Cs["logits"], S, axis=0) + g64).argmax(axis=1), Cs["argmax"])
    ys, dy = Cs["y_soft"], Cl["dy"]
    da = ys * (dy - (ys * dy).sum(axis=1, keepdims=True))
    want = (da / tau).reshape(B, S, K).sum(axis=1) + Cl["dlogits"]          # (the leaf run's dlogits: the entropy term alone)
    assert np.abs(want - Cs["dlogits"]).max() <= 1e-12 * max(np.abs(want).max(), 1e-30)
    # the generative gradients are those at the leaf y_hard; the y encoder's differ from the relaxed step's
    for k in gs:
        if not k.startswith("encoder_y"):
            assert np.abs(gs[k] - gl[k]).max() <= 1e-13 * max(np.abs(gl[k]).max(), 1.0), k
    C2, _ = TR.loss_and_grads(d, p, x, eps, u, 3.0 * tau, straight_through=True, weights=w)
    assert C2["loss"] == Cs["loss"] and np.array_equal(C2["y"], Cs["y"])
    Cr, gr = TR.loss_and_grads(d, p, x, eps, u, tau, weights=w)
    assert abs(Cr["loss"] - Cs["loss"]) > 1e-6 * abs(Cs["loss"])
    assert np.abs(gr["encoder_y_fcnet/linear_0/w"] - gs["encoder_y_fcnet/linear_0/w"]).max() > 0


@pytest.mark.parametrize("name", list(TR.CASES))
def test_top_two_gap_of_the_gpu_cases(name):
    """The condition tests/test_ytemp.py relies on: every row's two largest logits + g differ by more than MIN_GAP, so the
    device's fp32 argmax is the fp64 one."""
    d, p, flat, x, eps, u = TR.setup(name)
    C0, _ = TR.loss_and_grads(d, p, x, eps, u, 1.0, straight_through=True, weights=TR.case_weights(name))
    print(f"{name}: smallest top-two gap {C0['gap'].min():.4e}")
    assert C0["gap"].min() > TR.MIN_GAP


# ------------------------------------------------------------------------------------------------ the library
def test_flag_values_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    for cname, val, got in (("GMVAE_Y_TEMP_DEV", 128, L.Y_TEMP_DEV), ("GMVAE_Y_STRAIGHT_THROUGH", 256, L.Y_STRAIGHT_THROUGH)):
        m = re.search(cname + r"\s*=\s*(\d+)", hdr)
        assert m and int(m.group(1)) == got == val
    others = (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG | L.OBJ_LABELS |
              L.OBJ_WEIGHTS)
    assert (L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH) & others == 0 and L.Y_TEMP_DEV & L.Y_STRAIGHT_THROUGH == 0
    assert L.Y_ESTIMATORS == ("relaxed", "straight_through")
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


def _offset(L, d, model, name):
    o = C.c_uint64()
    return L.lib.gmvae_workspace_offset(C.byref(d), model, name, C.byref(o)), o.value


def _bytes(L, d, model):
    n = C.c_uint64()
    return L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(n)), n.value


WS_DIMS = [   # (B, D, Lz, K, hidden, S, other flags)
    (1024, 784, 64, 10, (64,), 1, 0), (1024, 784, 64, 10, (64,), 10, 0), (3, 100, 5, 7, (24, 24), 3, 0), (5, 64, 8, 17, (16,), 1, 0),
    (5, 128, 8, 65, (64,), 2, 0), (8, 100, 5, 7, (24, 24), 1, 64), (1024, 784, 64, 10, (64,), 1, 1),
]
OLD_NAMES = [b"y", b"logits", b"dlogits", b"dy", b"z", b"qp", b"pp", b"slabs", b"eps", b"u"]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"B{c[0]}-K{c[3]}-S{c[5]}-f{c[6]}")
def test_workspace_grows_behind_everything(L, case):
    """+temp: exactly 256 bytes (32 floats, rounded up), "y_temperature" where the workspace without the bits ended.  +st:
    r256(4 R K) more, "y_soft" behind the temperatures.  No other offset moves; without the bits both names are GMVAE_E_NET."""
    B, D, Lz, K, hidden, S, fl = case
    model = L.MODEL_IDS["gmvae"]
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=fl | f)
    rc0, n0 = _bytes(L, mk(0), model)
    assert rc0 == 0
    assert _offset(L, mk(0), model, b"y_temperature")[0] == E_NET == _offset(L, mk(0), model, b"y_soft")[0]
    ysoft = r256(4 * B * S * K)
    ends = set()
    for f, grow in ((L.Y_TEMP_DEV, 256), (L.Y_STRAIGHT_THROUGH, ysoft), (L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH, 256 + ysoft)):
        rc, n = _bytes(L, mk(f), model)
        assert rc == 0 and n == n0 + grow, (f, n, n0, grow)
        for nm in OLD_NAMES:
            assert _offset(L, mk(f), model, nm) == _offset(L, mk(0), model, nm), nm
        if fl & L.OBJ_WEIGHTS:
            assert _offset(L, mk(f), model, b"obj_weights") == _offset(L, mk(0), model, b"obj_weights")
        t, s = _offset(L, mk(f), model, b"y_temperature"), _offset(L, mk(f), model, b"y_soft")
        ends.add(min(o for rc_, o in (t, s) if rc_ == 0))
        behind = OLD_NAMES + ([b"obj_weights", b"rwk", b"y_floor"] if fl & L.OBJ_WEIGHTS else [])
        last = max(_offset(L, mk(0), model, nm)[1] for nm in behind)
        if f & L.Y_TEMP_DEV:
            assert t[0] == 0 and last < t[1] <= n0 and t[1] % 256 == 0 and t[1] + 256 <= n
        else:
            assert t == (E_NET, 0)
        if f & L.Y_STRAIGHT_THROUGH:
            assert s[0] == 0 and last < s[1] and s[1] + ysoft <= n
            assert not f & L.Y_TEMP_DEV or s[1] == t[1] + 256
        else:
            assert s == (E_NET, 0)
    assert len(ends) == 1          # (the new regions start where the layout without the bits ends, whichever bit is set)


def test_refusals_come_from_workspace_bytes(L):
    gm, vae, gmp = (L.MODEL_IDS[m] for m in ("gmvae", "vae", "vae_gmp"))
    for bit in (L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH, L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH):
        mk = lambda f, S=1, K=7: L.make_dims(8, 100, 5, K, (24, 24), S=S, sched_flags=bit | f)
        assert _bytes(L, mk(0), gm)[0] == 0 and _bytes(L, mk(0, S=3), gm)[0] == 0
        assert _bytes(L, mk(L.OBJ_WEIGHTS), gm)[0] == 0                          # (combines with the weighted objective at S == 1)
        assert _bytes(L, mk(L.OBJ_WEIGHTS, S=3), gm)[0] == E_DIMS             # (whose own refusal stays)
        assert _bytes(L, mk(0, K=1), vae)[0] == E_MODEL and _bytes(L, mk(0, K=3), gmp)[0] == E_MODEL
        assert _bytes(L, mk(L.OBJ_MARGINAL_Y), gm)[0] == E_DIMS
        assert _bytes(L, mk(L.OBJ_MARGINAL_Y_IW, S=3), gm)[0] == E_DIMS
        assert _bytes(L, mk(L.OBJ_MARGINAL_Y | L.OBJ_LABELS), gm)[0] == E_DIMS
        assert _bytes(L, mk(L.OBJ_MARGINAL_Y | L.GRAD_DREG), gm)[0] == E_DIMS
        assert _bytes(L, mk(L.GRAD_DREG), gm)[0] == E_DIMS
        # the evaluators mask the bits: their sizes are those without them
        for q in (L.iw_bound_workspace_bytes, L.iw_bound_enum_y_workspace_bytes, L.posterior_y_workspace_bytes):
            assert q(mk(0, S=3), gm) == q(L.make_dims(8, 100, 5, 7, (24, 24), S=3), gm)


SCHED = [   # (B, D, Lz, K, hidden, S, schedule without the bits)
    (1024, 784, 64, 10, (64,), 1, None), (24, 128, 8, 65, (64,), 1, "general"), (5, 128, 8, 65, (64,), 2, "general"),
    (64, 784, 128, 10, (512,), 1, None), (3, 100, 5, 7, (24, 24), 3, "general"),
]


@pytest.mark.parametrize("case", SCHED, ids=lambda c: f"B{c[0]}-K{c[3]}-S{c[5]}")
def test_schedule_names(L, case):
    """A step with either bit takes the general schedule; "+temp" then "+st" stand behind "+weights"; without the bits the
    schedule is what it was (one-launch at the reference's default sizes)."""
    B, D, Lz, K, hidden, S, base = case
    gm = L.MODEL_IDS["gmvae"]
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=f)
    s0 = L.step_schedule(mk(0), gm)
    if base is not None:
        assert s0 == base
    else:
        assert not s0.startswith("general")
    tail = "+planes" if s0.endswith("+planes") else ""
    gen = L.step_schedule(mk(L.Y_TEMP_DEV), gm)
    assert gen.startswith("general+temp") and "+st" not in gen
    pl = gen[len("general+temp"):]
    assert pl in ("", "+planes")
    assert L.step_schedule(mk(L.Y_STRAIGHT_THROUGH), gm) == "general+st" + pl
    assert L.step_schedule(mk(L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH), gm) == "general+temp+st" + pl
    if S == 1:
        assert L.step_schedule(mk(L.OBJ_WEIGHTS | L.Y_TEMP_DEV), gm) == "general+weights+temp" + pl
        assert L.step_schedule(mk(L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH), gm) == "general+weights+temp+st" + pl
    assert L.step_schedule(mk(0), gm) == s0 and (not tail or s0.startswith("general"))


# ------------------------------------------------------------------------------------------------ Python surface
def _cfg(**kw):
    base = dict(temperature=1.0, temperature_min=0.0, temperature_anneal_rate=0.0, temperature_anneal_every=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_temperature_at_corners():
    from gmvae_amd import runners
    import math
    c = _cfg(temperature=2.0, temperature_min=0.5, temperature_anneal_rate=0.1, temperature_anneal_every=4)
    N, r = 4, 0.1
    assert runners.temperature_at(c, 0) == 2.0 == runners.temperature_at(c, N - 1)
    assert runners.temperature_at(c, N) == 2.0 * math.exp(-r * N) == runners.temperature_at(c, 2 * N - 1)
    assert runners.temperature_at(c, 2 * N) == 2.0 * math.exp(-r * N * 2)
    # the step where the floor takes over: the first block index j with 2 exp(-r N j) <= 0.5, j = ceil(ln 4 / (r N)) = 4
    j = math.ceil(math.log(2.0 / 0.5) / (r * N))
    assert j == 4
    assert runners.temperature_at(c, j * N - 1) == 2.0 * math.exp(-r * N * (j - 1)) > 0.5
    assert runners.temperature_at(c, j * N) == 0.5 == runners.temperature_at(c, 10 ** 9)
    for n in (0, -3):                                          # N <= 0: no annealing
        cn = _cfg(temperature=2.0, temperature_min=0.5, temperature_anneal_rate=0.1, temperature_anneal_every=n)
        assert runners.temperature_at(cn, 0) == runners.temperature_at(cn, 1000) == 2.0
    assert runners.temperature_at(_cfg(temperature=0.25, temperature_min=0.5), 7) == 0.5
    assert runners.temperature_at(types.SimpleNamespace(), 5) == 1.0                       # (no flags at all: the reference's 1.0)
    assert not runners.temperature_flags(types.SimpleNamespace()) and not runners.temperature_flags(_cfg())
    for k, v in (("temperature", 0.7), ("temperature_min", 0.5), ("temperature_anneal_rate", 0.01), ("temperature_anneal_every", 2)):
        assert runners.temperature_flags(_cfg(**{k: v})), k


def test_engine_argument_check():
    from gmvae_amd.engine import check_y_head
    check_y_head("gmvae", "gumbel", 0.5, True, "straight_through")
    check_y_head("gmvae", "gumbel", 1.0, False, "relaxed")
    check_y_head("vae", "gumbel", 1.0, False, "relaxed")
    check_y_head("gmvae", "marginal", 1.0, False, "relaxed")
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            check_y_head("gmvae", "gumbel", t, True, "relaxed")
    with pytest.raises(ValueError, match="y_estimator"):
        check_y_head("gmvae", "gumbel", 1.0, False, "hard")
    for model in ("vae", "vae_gmp"):
        with pytest.raises(ValueError, match="GMVAE"):
            check_y_head(model, "gumbel", 1.0, True, "relaxed")
        with pytest.raises(ValueError, match="GMVAE"):
            check_y_head(model, "gumbel", 1.0, False, "straight_through")
    for yi in ("marginal", "marginal_iw"):
        with pytest.raises(ValueError, match="gumbel"):
            check_y_head("gmvae", yi, 1.0, True, "relaxed")
        with pytest.raises(ValueError, match="gumbel"):
            check_y_head("gmvae", yi, 1.0, False, "straight_through")


def test_cli_flags():
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args(["--model=gmvae"]))
    assert (cfg.temperature, cfg.temperature_min, cfg.temperature_anneal_rate, cfg.temperature_anneal_every,
            cfg.y_estimator) == (1.0, 0.0, 0.0, 0, "relaxed")
    assert not runners.temperature_flags(cfg)
    ok = run_gmvae.check_args(p, p.parse_args(["--model=gmvae", "--temperature=2", "--temperature_min=0.5",
                                               "--temperature_anneal_rate=0.03", "--temperature_anneal_every=2",
                                               "--y_estimator=straight_through"]))
    assert runners.temperature_flags(ok) and ok.y_estimator == "straight_through"
    bad = [["--model=vae", "--temperature=2"], ["--model=vae_gmp", "--y_estimator=straight_through"],
           ["--model=gmvae", "--y_inference=marginal", "--temperature_anneal_every=2"],
           ["--model=gmvae", "--y_inference=marginal_iw", "--y_estimator=straight_through"],
           ["--model=gmvae", "--temperature=0"], ["--model=gmvae", "--temperature_min=-1"],
           ["--model=gmvae", "--temperature_anneal_rate=0.1", "--temperature_anneal_every=2"]]
    for args in bad:
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(args))


def test_relaxed_one_hot_sample_follows_the_estimator():
    """base.RelaxedOneHotCategorical.sample: softmax((logits + g) / T), or the one-hot argmax of logits + g (first index on a
    tie) under straight_through."""
    import torch
    from gmvae_amd import base
    lg = torch.tensor([[0.0, 1.0, 1.0, -2.0], [3.0, 0.0, 0.0, 0.0]])
    uu = torch.full((2, 4), 0.5)
    soft = base.RelaxedOneHotCategorical(0.5, lg).sample(uniform=uu)
    g = -torch.log(-torch.log(uu))
    assert torch.allclose(soft, torch.softmax((lg + g) / 0.5, -1))
    hard = base.RelaxedOneHotCategorical(0.5, lg, straight_through=True).sample(uniform=uu)
    assert torch.equal(hard, torch.tensor([[0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]]))
