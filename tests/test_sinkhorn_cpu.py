"""gmvae_amd.sinkhorn without a GPU: the statement (tests/sinkhorn_ref.py) against answers worked by hand; the form the device takes
(the centred expanded square in fp64) against it on every device shape; the p-value's tie rule; the schedule; the library's argument
checks and workspace size through the ABI; the Python and runner gates."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import sinkhorn_cases as K
import sinkhorn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_sinkhorn_workspace_bytes", "gmvae_sinkhorn"}
E_NULL, E_DIMS, E_ALIGN = -1, -2, -4
PTR = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch
FORM_MARGIN = 100.0      # the form's error must sit this many times below the device's gate


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def converged(x, y, blur_rel, T, a=None, b=None, n_final=None):
    z = np.concatenate([x, y])
    out = R.divergence(x, y, R.schedule(z, T, blur_rel=blur_rel, n_final=n_final), a, b)
    return out, R.cscale(z)


# ------------------------------------------------------------------------------------------------------------ the statement
def test_two_single_points_give_the_cost():
    """n = m = 1: p and q stay 0, f' = C - g, so S = f' + g = C whatever the schedule."""
    rng = np.random.default_rng(1)
    for D in (1, 3, 784):
        x, y = rng.standard_normal((1, D)).astype(np.float32), rng.standard_normal((1, D)).astype(np.float32)
        cost = float(0.5 * ((x.astype(R.LD) - y.astype(R.LD)) ** 2).sum())
        out, _ = converged(x, y, 0.1, 5)
        print(f"D = {D}: S = {out['sinkhorn']!r}, C = {cost!r}")
        assert abs(out["sinkhorn"] - cost) <= 4 * np.finfo(np.float64).eps * cost
        assert out["marginal_err"] <= 1e-15 and not out["p"].any() and not out["q"].any()


def test_a_sample_against_itself_gives_zero():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((7, 2)).astype(np.float32)
    a = rng.uniform(0.5, 1.5, 7)
    a /= a.sum()
    for w in (None, a):
        out, scale = converged(x, x.copy(), 0.3, 2000, w, w, n_final=1800)
        print(f"S = {out['sinkhorn']:.3e} = {out['sinkhorn'] / scale:.3e} cscale, marginal_err = {out['marginal_err']:.3e}")
        assert out["marginal_err"] < 1e-12
        assert abs(out["sinkhorn"]) <= 1e-9 * scale


def assignment_cost(cost):
    """The least mean cost of a one-to-one assignment (scipy's linear_sum_assignment; without scipy, every permutation)."""
    try:
        from scipy.optimize import linear_sum_assignment
        r, c = linear_sum_assignment(cost)
        return float(cost[r, c].mean())
    except ImportError:
        n = len(cost)
        perms = np.array(list(itertools.permutations(range(n))))
        return float(cost[np.arange(n)[None, :], perms].mean(axis=1).min())


def test_small_blur_gives_the_assignment_cost():
    """Eight points a side, uniform weights, blur_rel = 0.02: the entropic term is gone and the self-terms with it, so S is the
    optimal transport cost, which for uniform weights at n = m is the best one-to-one assignment's mean cost.  What is left is
    exp(-gap / eps) -- the gap to the next best assignment, and between neighbours within a sample --, so the seed is one whose
    points lie several blurs apart (of the seeds 30 .. 41 a third give 0 to rounding, the others 1e-8 .. 5e-5 cscale)."""
    rng = np.random.default_rng(35)
    x, y = rng.standard_normal((8, 2)).astype(np.float32), (0.5 + rng.standard_normal((8, 2))).astype(np.float32)
    out, scale = converged(x, y, 0.02, 400)
    cost = np.asarray(0.5 * ((x.astype(R.LD)[:, None, :] - y.astype(R.LD)[None, :, :]) ** 2).sum(axis=2), dtype=np.float64)
    best = assignment_cost(cost)
    print(f"S = {out['sinkhorn']!r}, assignment = {best!r}, difference = {abs(out['sinkhorn'] - best) / scale:.3e} cscale, "
          f"marginal_err = {out['marginal_err']:.3e}")
    assert abs(out["sinkhorn"] - best) <= 1e-9 * scale


def test_swapping_the_samples_swaps_the_outputs():
    """Run to convergence (the iteration updates f first, so only its fixed point is symmetric): S is the same, and the per-point
    contributions change sides -- up to the constant the potentials are determined up to (f + c, g - c), which the fixed point of
    the iteration picks by where it starts."""
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal((6, 2)).astype(np.float32), (0.4 + rng.standard_normal((9, 2))).astype(np.float32)
    one, scale = converged(x, y, 0.3, 600)
    two, _ = converged(y, x, 0.3, 600)
    assert one["marginal_err"] < 1e-12 and two["marginal_err"] < 1e-12
    c = (two["contrib_y"] - one["contrib_x"]).mean()
    worst = max(abs(one["sinkhorn"] - two["sinkhorn"]), abs(one["part_x"] + one["part_y"] - two["part_x"] - two["part_y"]),
                np.abs(two["contrib_y"] - one["contrib_x"] - c).max(), np.abs(two["contrib_x"] - one["contrib_y"] + c).max(),
                np.abs(two["q"] - one["p"]).max(), np.abs(two["p"] - one["q"]).max())
    print(f"worst difference = {worst / scale:.3e} cscale (c = {c:.3e})")
    assert worst <= 1e-12 * scale


@pytest.mark.parametrize("kind", K.WEIGHTS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_the_devices_form_matches_the_statement(shape, kind):
    """The centred expanded square in fp64, clamped, with C_ii = 0 on the symmetric problems and every sum in fp64 -- the form the
    statement allows the device -- against differences and sums in longdouble: at least FORM_MARGIN times below the device's gate
    (measured: 1.7e-5 of the gate at worst, profiles/sinkhorn_notes.md)."""
    ref, got, scale = K.reference(shape, kind), K.reference(shape, kind, "expanded"), K.scale(shape)
    err = max(np.abs(np.asarray(ref[k]) - np.asarray(got[k])).max()
              for k in ("f", "g", "p", "q", "contrib_x", "contrib_y", "sinkhorn", "part_x", "part_y"))
    merr = abs(ref["marginal_err"] - got["marginal_err"]) / (1.0 + ref["marginal_err"])
    print(f"{shape} {kind}: form error = {err / (R.GATE * scale):.3e} of the gate; marginal_err {ref['marginal_err']:.3e}, relative "
          f"difference {merr:.3e}")
    assert err <= R.GATE * scale / FORM_MARGIN
    assert merr <= 2 * R.GATE * scale / K.eps(shape)[-1] / FORM_MARGIN


def test_the_schedule():
    rng = np.random.default_rng(5)
    z = (3.0 + rng.standard_normal((40, 5))).astype(np.float32)
    rms = R.rms_distance(z)
    d = np.sqrt(((z.astype(np.float64)[:, None] - z.astype(np.float64)[None]) ** 2).sum(axis=2))
    assert abs(rms - np.sqrt((d ** 2).sum() / (40 * 39))) <= 1e-12 * rms
    eps = R.schedule(z, 12, blur_rel=0.2, n_final=3)
    r = np.sqrt(((z - z.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1).max())
    assert eps.shape == (13,) and abs(eps[0] - 4 * r * r) <= 1e-12 * eps[0] and (eps[9:] == (0.2 * rms) ** 2).all()
    ratio = eps[1:10] / eps[:9]
    assert np.abs(ratio - ratio[0]).max() <= 1e-12 and ratio[0] < 1.0
    assert np.abs(R.schedule(z, 12, blur=100.0, n_final=3) / 1e4 - 1.0).max() <= 1e-14      # a blur wider than the sample: eps[0] = eps[T]
    assert (R.schedule(z, 4, blur_rel=0.2, n_final=4) == eps[-1]).all()       # nothing but final entries
    assert R.schedule(z, 200).shape == (201,) and R.schedule(z, 200)[150] == R.schedule(z, 200)[200] < R.schedule(z, 200)[149]


def test_the_p_value_counts_ties():
    """Two distinct points u and v: S depends on a split only through how many u its first sample holds, so splits tie with the
    observed one -- to rounding, the rows being in another order -- and the rule (1 + #{null >= S - 1e-8 cscale}) / P counts them."""
    u, v = np.array([0.0, 0.0], dtype=np.float32), np.array([1.0, 0.5], dtype=np.float32)
    z = np.stack([u, u, u, v, u, v, v, v])
    rng = np.random.default_rng(6)
    P = 24
    splits = [np.arange(8) < 4] + [np.isin(np.arange(8), rng.permutation(8)[:4]) for _ in range(P - 1)]
    eps, scale = R.schedule(z, 20, blur_rel=0.3), R.cscale(z)
    S = np.array([R.divergence(z[e], z[~e], eps)["sinkhorn"] for e in splits])
    count = lambda e: int((z[e] == u).all(axis=1).sum())
    canon = {k: R.divergence(np.stack([u] * k + [v] * (4 - k)), np.stack([u] * (4 - k) + [v] * k), eps)["sinkhorn"] for k in range(5)}
    assert all(abs(S[i] - canon[count(e)]) <= 1e-12 * scale for i, e in enumerate(splits))
    gaps = sorted(canon.values())
    assert min(b - a for a, b in zip(gaps, gaps[1:]) if b - a > 1e-12 * scale) > 1e-3 * scale      # levels apart or equal: no edge case
    expected = sum(canon[count(e)] >= canon[3] - 1e-6 * scale for e in splits[1:])
    ties = sum(count(e) == 3 for e in splits[1:])
    print(f"S by the count of u: {canon}; {ties} of {P - 1} splits tie with the observed one, {expected} at or above it")
    assert count(splits[0]) == 3 and ties >= 2
    assert R.p_value(S[0], S[1:], scale) == (1.0 + expected) / P
    assert R.p_value(1.0, [1.0 - 0.5e-8, 1.0 - 2e-8, 1.0, 2.0], 1.0) == 4 / 5


# ------------------------------------------------------------------------------------------------------------ the library
def test_names_are_declared_exported_and_bound(L):
    header = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert L.lib.gmvae_abi_version() == L.ABI_VERSION == 7
    assert "twosample.hip" in open(os.path.join(ROOT, "build_hip.py")).read()


def wsb(L, n, m, D):
    b = C.c_uint64(0)
    return L.lib.gmvae_sinkhorn_workspace_bytes(n, m, D, C.byref(b)), b.value


BAD_SIZES = [(0, 4, 4), (4, 0, 4), (-3, 4, 4), ((1 << 20) + 1, 4, 4), (4, (1 << 20) + 1, 4), (1 << 32, 4, 4), (4, (1 << 32) + 1, 4),
             (8, 8, 0), (8, 8, 4097), (8, 8, -1)]


def test_workspace_size(L):
    for n, m, D in BAD_SIZES:
        assert wsb(L, n, m, D)[0] == E_DIMS, (n, m, D)
    assert L.lib.gmvae_sinkhorn_workspace_bytes(8, 4, 4, None) == E_NULL
    assert L.lib.gmvae_sinkhorn_workspace_bytes(0, 4, 4, None) == E_DIMS                     # the sizes come first
    for n, m, D in ((1, 1, 1), (1 << 20, 1 << 20, 4096), (1 << 20, 1, 1), (1, 1 << 20, 4096), (1537, 800, 8), (10000, 10000, 784),
                    (8200, 70, 4)):
        rc, b = wsb(L, n, m, D)
        assert rc == 0 and b % 16 == 0 and b == wsb(L, n, m, D)[1]
        # a (max, sum) pair per row, problem and slab -- at most 16 slabs --, three doubles a row and at most 65 D for the mean
        assert 0 < b <= 8 * (2 * 3 * 16 * max(n, m) + 3 * (n + m) + 2 + 65 * D) + 16, (n, m, D, b)
    # (from 1024 rows on, where the 16 slabs are reached: below, the slabs grow with the column tiles, the bound above holding)
    for n, m, D in ((1100, 1500, 16), (5000, 7000, 64), (20000, 20000, 784), (1 << 19, 1 << 18, 8)):
        one, two = wsb(L, n, m, D)[1], wsb(L, 2 * n, 2 * m, D)[1]
        print(f"({n}, {m}, {D}): {one} bytes, doubled {two}: {two / one:.3f} times")
        assert two <= 2.05 * one                                                             # O(n + m): never n m
    assert wsb(L, 10000, 10000, 784)[1] < 8 * 10000 * 10000 // 100
    from gmvae_amd import sinkhorn
    assert sinkhorn.workspace_bytes(1537, 800, 8) == wsb(L, 1537, 800, 8)[1]


def _p(a):
    return None if a is None else C.c_void_p(a)


def call(L, x=PTR, n=64, y=PTR, m=48, D=4, a=PTR, b=PTR, eps=PTR, n_iter=5, f=PTR, g=PTR, p=PTR, q=PTR, out=PTR, ws=PTR):
    return L.lib.gmvae_sinkhorn(_p(x), n, _p(y), m, D, _p(a), _p(b), _p(eps), n_iter, _p(f), _p(g), _p(p), _p(q), _p(out), _p(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for n, m, D in BAD_SIZES:
        assert call(L, n=n, m=m, D=D) == E_DIMS, (n, m, D)
    for n_iter in (0, -1, 100001):
        assert call(L, n_iter=n_iter) == E_DIMS
    required = ("x", "y", "eps", "f", "g", "p", "q", "out", "ws")
    for name in required:
        assert call(L, **{name: None}) == E_NULL, name
        assert call(L, **{name: None}, n=0) == E_DIMS and call(L, **{name: None}, n_iter=0) == E_DIMS, name      # the sizes come first
    for name, off in (("x", 2), ("y", 2), ("a", 4), ("b", 4), ("eps", 4), ("f", 4), ("g", 4), ("p", 4), ("q", 4), ("out", 4), ("ws", 8)):
        assert call(L, **{name: PTR + off}) == E_ALIGN, name
        assert call(L, **{name: PTR + off}, **{"y" if name == "x" else "x": None}) == E_NULL, name              # NULL before the alignment
    # every edge of the gate passes the size check (and fails the next one); the weights may be NULL
    for kw in ({"n": 1, "m": 1, "D": 1, "n_iter": 1}, {"n": 1 << 20, "m": 1 << 20, "D": 4096, "n_iter": 100000}):
        assert call(L, **kw, x=None) == E_NULL and call(L, **kw, ws=PTR + 8) == E_ALIGN
    assert call(L, a=None, b=None, ws=PTR + 8) == E_ALIGN and call(L, a=None, b=None, out=None) == E_NULL


def test_python_gate_raises_value_errors(L, monkeypatch):
    """gmvae_amd.sinkhorn refuses what the library would, and a blur that is no blur, as ValueError before any launch; the
    schedule it builds is the statement's."""
    import torch
    from gmvae_amd import sinkhorn, twosample
    monkeypatch.setattr(twosample, "_rows", lambda x, what: torch.as_tensor(x, dtype=torch.float32))
    x, y = torch.randn(8, 4), torch.randn(6, 4)
    for fn in (sinkhorn.divergence, sinkhorn.divergence_test):
        for kw in ({"blur": 0.0}, {"blur": -1.0}, {"blur": float("nan")}, {"blur": float("inf")}, {"blur_rel": 0.0},
                   {"blur_rel": float("nan")}, {"n_iter": 0}, {"n_iter": 100001}, {"n_iter": 10, "n_final": 11}, {"n_iter": 10, "n_final": -1}):
            with pytest.raises(ValueError):
                fn(x, y, **kw)
        with pytest.raises(ValueError):
            fn(x, torch.randn(6, 5))
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 4097), torch.zeros(2, 4097))
        with pytest.raises(ValueError):
            fn(torch.zeros(0, 4), y)
    for P in (0, 4097):
        with pytest.raises(ValueError):
            sinkhorn.divergence_test(x, y, n_perms=P)
    for bad in ((0, 4, 4), (4, 0, 4), ((1 << 20) + 1, 4, 4), (4, (1 << 20) + 1, 4), (8, 8, 0), (8, 8, 4097), (8, 8, 4, 0), (8, 8, 4, 100001)):
        with pytest.raises(ValueError):
            sinkhorn.check_sizes(*bad)
    sinkhorn.check_sizes(1, 1, 1, 1)
    sinkhorn.check_sizes(1 << 20, 1 << 20, 4096, 100000)
    for bad in ({"eps": torch.ones(1, dtype=torch.float64)}, {"eps": torch.ones(2, 2, dtype=torch.float64)},
                {"eps": torch.ones(3, dtype=torch.float64), "a": torch.ones(7, dtype=torch.float64)},
                {"eps": torch.ones(3, dtype=torch.float64), "b": torch.ones(8, dtype=torch.float64)}):
        with pytest.raises(ValueError):
            sinkhorn.solve(x, y, **bad)
    z = torch.from_numpy((3.0 + np.random.default_rng(7).standard_normal((50, 6))).astype(np.float32))
    for kw in ({"n_iter": 12, "blur_rel": 0.2, "n_final": 3}, {"n_iter": 200}, {"n_iter": 7, "blur": 0.5}, {"n_iter": 5, "blur": 1e3},
               {"n_iter": 4, "n_final": 4}):
        got, ref = sinkhorn.schedule(z, **kw).numpy(), R.schedule(z.numpy(), **kw)
        assert got.dtype == np.float64 and got.shape == ref.shape and np.abs(got / ref - 1.0).max() <= 1e-12, kw


def test_runner_flag_checks(L, monkeypatch):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_distance=64", "--sample_distance_space=both", "--sinkhorn_blur_rel=0.2",
                                               "--sinkhorn_iters=50", "--sample_distance_perms=20"]))
    assert (ok.sample_distance, ok.sample_distance_space, ok.sinkhorn_blur_rel, ok.sinkhorn_iters, ok.sample_distance_perms) == \
        (64, "both", 0.2, 50, 20)
    plain = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_distance=2"]))
    assert (plain.sample_distance_space, plain.sinkhorn_blur_rel, plain.sinkhorn_iters, plain.sample_distance_perms) == ("data", 0.1, 200, 0)
    grey = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_distance=64", "--sample_distance_space=code",
                                                 "--likelihood=continuous_bernoulli"]))      # the code space takes any likelihood
    assert grey.sample_distance_space == "code"
    with_test = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_distance=64", "--sample_test=64"]))
    assert with_test.sample_test == 64 and with_test.sample_distance == 64
    d = ["--mode=eval", "--sample_distance=64"]
    for bad in (["--mode=train", "--sample_distance=64"], ["--mode=eval", "--sample_distance=-1"], ["--mode=eval", "--sample_distance=1"],
                ["--mode=eval", f"--sample_distance={(1 << 20) + 1}"],
                ["--mode=eval", "--sample_distance_perms=10"], ["--mode=eval", "--sample_distance_space=code"],
                ["--mode=eval", "--sinkhorn_blur_rel=0.2"], ["--mode=eval", "--sinkhorn_iters=50"],
                ["--mode=eval", "--sample_test=64", "--sinkhorn_iters=50"],
                d + ["--sample_distance_perms=-1"], d + ["--sample_distance_perms=4097"], d + ["--sample_distance_space=x"],
                d + ["--sinkhorn_iters=0"], d + ["--sinkhorn_iters=100001"], d + ["--sinkhorn_blur_rel=0"], d + ["--sinkhorn_blur_rel=-0.1"],
                d + ["--sinkhorn_blur_rel=nan"], d + ["--sinkhorn_blur_rel=inf"],
                d + ["--likelihood=continuous_bernoulli"], d + ["--sample_distance_space=both", "--likelihood=gaussian"],
                d + ["--sample_distance_space=code", "--missing_rate=0.2"], d + ["--missing_rate=0.2"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        run_gmvae.check_args(p, p.parse_args(d))
