"""gmvae_amd.twosample without a GPU: the statement (tests/twosample_ref.py) against answers worked by hand and its own invariants;
the two forms of the squared distance; that the p-value rule leaves no split of the device cases undecided; the library's argument
checks and workspace size through the ABI; the Python and runner gates."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import twosample_cases as K
import twosample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_mmd_workspace_bytes", "gmvae_mmd"}
E_NULL, E_DIMS, E_MODEL, E_ALIGN = -1, -2, -3, -4
PTR = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------ the statement
def test_known_answers_for_two_points_a_sample():
    """x = {0, 1}, y = {2, 4} on the line.  Energy: 2 E|X - Y| - E|X - X'| - E|Y - Y'| = 2 * 2.5 - 1 - 2 = 2.  rbf with gamma = ln 2,
    k = 2^-d2: the pairs within give 1/2 and 1/16, the four across 2^-4, 2^-16, 2^-1, 2^-9."""
    z = np.array([[0.0], [1.0], [2.0], [4.0]], dtype=np.float32)
    E = np.array([[1, 1, 0, 0]], dtype=np.uint8)
    got, row_all, row_first = R.mmd(z, E, "energy")
    assert abs(got[0] - 2.0) <= 1e-15
    assert np.array_equal(row_all, -np.array([7.0, 5.0, 5.0, 9.0])) and np.array_equal(row_first, -np.array([1.0, 1.0, 3.0, 7.0]))
    assert np.allclose(R.witness(row_all, row_first, E[0]), [-1 + 3, -1 + 2, -1.5 + 2, -3.5 + 2], atol=1e-15)
    got, row_all, row_first = R.mmd(z, E, "rbf", [math.log(2.0)])
    cross = 2.0 ** -4 + 2.0 ** -16 + 2.0 ** -1 + 2.0 ** -9
    assert abs(got[0] - (0.5 + 1.0 / 16 - 2.0 * cross / 4)) <= 1e-15
    assert abs(row_first[2] - (2.0 ** -4 + 2.0 ** -1)) <= 1e-15 and abs(row_all[0] - (0.5 + 2.0 ** -4 + 2.0 ** -16)) <= 1e-15
    # a mixture of bandwidths is the mean of the kernels; a split with one point on a side has no unbiased estimate
    two = R.mmd(z, E, "rbf", [math.log(2.0), 0.0])[0][0]
    assert abs(two - 0.5 * got[0]) <= 1e-15                          # (gamma = 0: k = 1 everywhere, whose mmd2 is 0)
    assert np.isnan(R.mmd(z, np.array([[1, 0, 0, 0], [1, 1, 1, 0]]), "energy")[0]).all()
    assert R.kscale(z, "rbf") == 1.0 and abs(R.kscale(z, "energy") - math.sqrt((1 + 4 + 16 + 1 + 9 + 4) / 6)) <= 1e-15


@pytest.mark.parametrize("kernel", ["rbf", "energy"])
def test_unbiased_statistic_sums_to_zero_over_all_splits(kernel):
    rng = np.random.default_rng(5)
    z = rng.standard_normal((6, 3)).astype(np.float32)
    E = np.zeros((20, 6), dtype=np.uint8)
    for p, idx in enumerate(itertools.combinations(range(6), 3)):
        E[p, list(idx)] = 1
    got = R.mmd(z, E, kernel, R.gammas(2.0))[0]
    print(f"{kernel}: the 20 splits sum to {got.sum():.3e}, the largest {np.abs(got).max():.3e}")
    assert abs(got.sum()) <= 1e-13 * np.abs(got).max() * 20


def test_p_value_counts_ties_and_ignores_nan():
    m = np.array([0.5, 0.5, 0.5 - 0.9e-8, 0.5 - 1.1e-8, np.nan, 0.7, 0.1])
    assert R.p_value(m, 1.0) == (1 + 3) / 7
    count, undecided = R.exceedances(m, 1.0)
    assert count == 2 and undecided.tolist() == [False, True, True, False, False, False]


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_difference_and_expanded_forms_agree(shape):
    """The centred expanded square in fp64 -- the form a kernel may take for rbf -- against the differences in longdouble: mmd2 and
    the row sums over N within 1e-3 of the device gate (1e-12), so summation order in fp64 sits far below that gate."""
    z, E = K.data(shape), K.splits(shape)
    N = z.shape[0]
    worst = 0.0
    for Q in (1, 3):
        a = R.mmd(z, E, "rbf", K.gamma(shape, Q), d2=K.sq_dists(shape))
        b = R.mmd(z, E, "rbf", K.gamma(shape, Q), d2=R.sq_dists_expanded(z))
        assert np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
        keep = ~np.isnan(a[0])
        worst = max(worst, np.abs(a[0][keep] - b[0][keep]).max() if keep.any() else 0.0, np.abs(a[1] - b[1]).max() / N,
                    np.abs(a[2] - b[2]).max() / N)
    print(f"{shape}: the two forms differ by {worst / R.GATE:.3e} of the gate")
    assert worst <= 1e-3 * R.GATE


@pytest.mark.parametrize("variant", K.VARIANTS, ids=K.vid)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_device_cases_leave_no_split_undecided(shape, variant):
    mmd2, _, _, scale = K.reference(shape, variant)
    n, m, D, P = shape
    nan = np.isnan(mmd2)
    sizes = (K.splits(shape) != 0).sum(axis=1)
    assert np.array_equal(nan, (sizes < 2) | (n + m - sizes < 2))
    count, undecided = R.exceedances(mmd2, scale)
    assert not undecided.any()
    if P > 5 and not nan[0]:
        assert count >= (2 if n == m else 1)                         # the copy of the observed split and, at n = m, its complement
        assert abs(mmd2[4] - mmd2[0]) <= 1e-12 * scale and (n != m or abs(mmd2[5] - mmd2[0]) <= 1e-12 * scale)


def test_the_tie_case_has_many_ties():
    mmd2, _, _, scale = K.reference(K.TIES, ("energy", 1))
    ties = (np.abs(mmd2[1:] - mmd2[0]) <= 1e-12 * scale).sum()
    print(f"{ties} of {len(mmd2) - 1} splits tie with the observed one")
    assert ties >= 10


def test_duplicated_rows_have_zero_energy_kernel():
    z = K.data(K.PIXELS)
    d2 = K.sq_dists(K.PIXELS)
    for i, j in K.DUPLICATES:
        assert np.array_equal(z[i], z[j]) and d2[i, j] == 0.0 and R.gram(d2, "energy")[i, j] == 0.0


def test_median_and_mean_bandwidths():
    z = np.array([[0.0], [1.0], [2.0], [4.0]], dtype=np.float32)
    assert R.median_distance(z) == 2.0                               # of 1, 1, 2, 2, 3, 4: the lower of the two middle ones
    rng = np.random.default_rng(9)
    z = rng.standard_normal((2500, 3)).astype(np.float32)
    sub = z[::3]                                                     # ceil(2500 / 1024) = 3
    d = np.sqrt(R.sq_dists(sub))[np.triu_indices(len(sub), 1)]
    assert R.median_distance(z) == np.sort(d)[(len(d) - 1) // 2]
    full = R.sq_dists(z[:300])
    assert abs(R.kscale(z[:300], "energy") - math.sqrt(full.sum() / (300 * 299))) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ the library
def test_names_are_declared_exported_and_bound(L):
    header = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert L.lib.gmvae_abi_version() == L.ABI_VERSION == 7
    assert "twosample.hip" in open(os.path.join(ROOT, "build_hip.py")).read()


def wsb(L, N, D, P):
    b = C.c_uint64(0)
    return L.lib.gmvae_mmd_workspace_bytes(N, D, P, C.byref(b)), b.value


BAD_SIZES = [(1, 4, 4), (0, 4, 4), (-3, 4, 4), ((1 << 20) + 1, 4, 4), (8, 0, 4), (8, 4097, 4), (8, 4, 0), (8, 4, 4097)]


def test_workspace_size(L):
    for N, D, P in BAD_SIZES:
        assert wsb(L, N, D, P)[0] == E_DIMS, (N, D, P)
    assert L.lib.gmvae_mmd_workspace_bytes(8, 4, 4, None) == E_NULL
    assert L.lib.gmvae_mmd_workspace_bytes(1, 4, 4, None) == E_DIMS                          # the sizes come first
    for N, D, P in ((2, 1, 1), (1 << 20, 4096, 4096), (1537, 8, 64), (20000, 784, 1000)):
        rc, b = wsb(L, N, D, P)
        assert rc == 0 and b % 16 == 0
        tiles = -(-N // 32)
        # O(N P) bytes plus O(tiles P) doubles, never N^2: at most 16 slabs of the row tiles' partials and of two row outputs, and
        # for the rbf kernel's centring at most 64 row slices of the mean, the mean and a norm per row
        assert 0 < b <= 8 * (16 * tiles * (2 * P + 1) + 2 * 16 * N + 65 * D + N) + 16, (N, D, P, b)
    assert wsb(L, 20000, 784, 1000)[1] < 8 * 20000 * 20000 // 100
    from gmvae_amd import twosample
    assert twosample.workspace_bytes(1537, 8, 64) == wsb(L, 1537, 8, 64)[1]


def _p(a):
    return None if a is None else C.c_void_p(a)


def call(L, z=PTR, N=64, D=4, assign=PTR, P=8, kernel=0, gamma=(1.0,), Q=None, mmd2=PTR, row_all=PTR, row_first=PTR, ws=PTR):
    g = None if gamma is None else (C.c_double * max(1, len(gamma)))(*gamma)
    Q = (0 if gamma is None else len(gamma)) if Q is None else Q
    return L.lib.gmvae_mmd(_p(z), N, D, _p(assign), P, kernel, g, Q, _p(mmd2), _p(row_all), _p(row_first), _p(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for N, D, P in BAD_SIZES:
        assert call(L, N=N, D=D, P=P) == E_DIMS, (N, D, P)
    for kind in (-1, 2, 7):
        assert call(L, kernel=kind) == E_MODEL and call(L, kernel=kind, N=1) == E_DIMS      # the sizes come first
    for Q in (0, 9, -1):
        assert call(L, Q=Q) == E_DIMS
    for g in (-1.0, float("nan"), float("inf")):
        assert call(L, gamma=(1.0, g)) == E_DIMS
    assert call(L, gamma=None, Q=1) == E_NULL
    assert call(L, kernel=1, gamma=None, Q=0, z=None) == E_NULL                               # energy: gamma and Q are not looked at,
    assert call(L, kernel=1, gamma=None, Q=99, ws=PTR + 8) == E_ALIGN                         # so the later checks are reached
    for name in ("z", "assign", "mmd2", "ws"):
        assert call(L, **{name: None}) == E_NULL, name
        assert call(L, **{name: None}, N=1) == E_DIMS, name
    for name, off in (("z", 2), ("mmd2", 4), ("row_all", 4), ("row_first", 4), ("ws", 8)):
        assert call(L, **{name: PTR + off}) == E_ALIGN, name
        assert call(L, **{name: PTR + off}, assign=None) == E_NULL, name                      # NULL before the alignment
    assert call(L, assign=PTR + 1, z=None) == E_NULL                                          # (bytes: no alignment asked of assign)
    # the gate's edges pass the size check (and fail the next one); the optional outputs may be NULL
    assert call(L, N=2, D=1, P=1, z=None) == E_NULL and call(L, N=1 << 20, D=4096, P=4096, gamma=(0.0,) * 8, z=None) == E_NULL
    assert call(L, row_all=None, row_first=None, z=None) == E_NULL


def test_python_gate_raises_value_errors(L, monkeypatch):
    """gmvae_amd.twosample refuses what the library would, as ValueError, before it asks for a device."""
    import torch
    from gmvae_amd import twosample
    monkeypatch.setattr(twosample, "_rows", lambda x, what: torch.as_tensor(x, dtype=torch.float32))
    x, y = torch.randn(8, 4), torch.randn(6, 4)
    for kw in ({"n_perms": 0}, {"n_perms": 4097}, {"kernel": "linear"}, {"bandwidth": "mode"}, {"bandwidth": 0.0},
               {"bandwidth": float("nan")}, {"bandwidth": [1.0] * 9}, {"bandwidth": []}, {"bandwidth": 1.0, "scales": [1.0] * 9},
               {"bandwidth": 1.0, "scales": [0.0]}, {"assignments": torch.zeros(4097, 14, dtype=torch.uint8), "bandwidth": 1.0}):
        with pytest.raises(ValueError):
            twosample.mmd_test(x, y, **kw)
    with pytest.raises(ValueError):
        twosample.mmd_test(x, torch.randn(6, 5), bandwidth=1.0)
    with pytest.raises(ValueError):
        twosample.mmd_test(torch.zeros(1, 4097), torch.zeros(1, 4097), bandwidth=1.0)
    with pytest.raises(ValueError):
        twosample.mmd_test(torch.zeros(3, 2), torch.zeros(3, 2), bandwidth="median")         # all rows equal: no bandwidth
    for bad in ((1, 4, 4), ((1 << 20) + 1, 4, 4), (8, 0, 4), (8, 4097, 4), (8, 4, 0), (8, 4, 4097)):
        with pytest.raises(ValueError):
            twosample.check_sizes(*bad)
    twosample.check_sizes(2, 1, 1)
    twosample.check_sizes(1 << 20, 4096, 4096, 8)
    # the permutations: row 0 the observed split, every row n points, the same rows for the same seed
    E = twosample.permutations(5, 7, 9, seed=3)
    assert E.dtype == torch.uint8 and E.shape == (9, 12) and E[0].tolist() == [1] * 5 + [0] * 7 and (E.sum(dim=1) == 5).all()
    assert torch.equal(E, twosample.permutations(5, 7, 9, seed=3)) and not torch.equal(E, twosample.permutations(5, 7, 9, seed=4))


def test_runner_flag_checks(L, monkeypatch):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_test=64", "--sample_test_perms=50", "--sample_test_kernel=energy",
                                               "--sample_test_space=both"]))
    assert (ok.sample_test, ok.sample_test_perms, ok.sample_test_kernel, ok.sample_test_space) == (64, 50, "energy", "both")
    plain = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_test=64"]))
    assert (plain.sample_test_perms, plain.sample_test_kernel, plain.sample_test_space) == (1000, "rbf", "data")
    grey = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_test=64", "--sample_test_space=code",
                                                 "--likelihood=continuous_bernoulli"]))      # the code space takes any likelihood
    assert grey.sample_test_space == "code"
    for bad in (["--mode=train", "--sample_test=64"], ["--mode=eval", "--sample_test=-1"], ["--mode=eval", "--sample_test=1"],
                ["--mode=eval", "--sample_test_perms=10"], ["--mode=eval", "--sample_test=64", "--sample_test_perms=0"],
                ["--mode=eval", "--sample_test=64", "--sample_test_perms=4097"], ["--mode=eval", "--sample_test=64", "--sample_test_kernel=x"],
                ["--mode=eval", "--sample_test=64", "--sample_test_space=x"],
                ["--mode=eval", "--sample_test=64", "--likelihood=continuous_bernoulli"],
                ["--mode=eval", "--sample_test=64", "--sample_test_space=both", "--likelihood=gaussian"],
                ["--mode=eval", "--sample_test=64", "--sample_test_space=code", "--missing_rate=0.2"],
                ["--mode=eval", "--sample_test=64", "--missing_rate=0.2"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--sample_test=64"]))
