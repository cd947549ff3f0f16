"""The statement of the neighbourhood scores (tests/neigh_ref.py) against scikit-learn, its tie and self rules on hand-made inputs,
and everything of gmvae_knn_* / gmvae_amd.neighbours / run_gmvae that is decided on the host: the workspace size, every gate's
return code, the ValueErrors, the flag checks.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import neigh_ref as R


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the statement vs scikit-learn
def _data(n=240, Lz=7, C_=5, seed=0):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C_, n)
    z = rng.normal(0, 1, (n, Lz)) + 1.5 * rng.normal(0, 1, (C_, Lz))[lab]
    return z.astype(np.float32), lab


def test_search_and_classifier_match_scikit_learn():
    nb = pytest.importorskip("sklearn.neighbors")
    z, lab = _data()
    q = _data(50, seed=1)[0]
    for k in (1, 5, 12):
        idx, d2 = R.search(q, z, k, key="fp64")
        sk_d, sk_i = nb.NearestNeighbors(n_neighbors=k, algorithm="brute").fit(z.astype(np.float64)).kneighbors(q.astype(np.float64))
        assert np.array_equal(idx, sk_i) and np.allclose(np.sqrt(d2), sk_d, rtol=1e-12)
        assert np.array_equal(R.search(q, z, k)[0], sk_i)                      # (no ties here: rounding d to fp32 moves nothing)
        pred, v = R.knn_classify(z, lab, q, k, 5)
        assert np.array_equal(pred, nb.KNeighborsClassifier(n_neighbors=k, algorithm="brute").fit(z.astype(np.float64), lab).predict(q.astype(np.float64)))
        assert (v.sum(axis=1) == k).all()
        # leave-one-out: the set against itself, self left out = scikit-learn's kneighbors() without an argument
        loo = R.search(z, z, k, self_offset=0)[0]
        assert np.array_equal(loo, nb.NearestNeighbors(n_neighbors=k, algorithm="brute").fit(z.astype(np.float64)).kneighbors()[1])
        assert np.array_equal(R.ranks(z, z, loo, 0), np.broadcast_to(np.arange(k), loo.shape))


def test_silhouette_trustworthiness_nmi_ari_match_scikit_learn():
    metrics = pytest.importorskip("sklearn.metrics")
    manifold = pytest.importorskip("sklearn.manifold")
    z, lab = _data()
    lab6 = lab.copy()
    lab6[0] = 5                                                                 # a class of one; class 6 stays empty
    for labels, C_ in ((lab, 5), (lab6, 7)):
        s, score = R.silhouette(z, labels, C_)
        ref = metrics.silhouette_samples(z.astype(np.float64), labels)
        print("silhouette", C_, np.abs(s - ref).max())
        assert np.abs(s - ref).max() <= 1e-9 and abs(score - ref.mean()) <= 1e-9
    assert s[0] == 0.0
    rng = np.random.default_rng(3)
    y = (z[:, :2] + 0.5 * rng.normal(0, 1, (z.shape[0], 2))).astype(np.float32)
    for k in (1, 5, 40):
        t = R.trustworthiness(z, y, k, key="fp64")             # (scikit-learn orders by the fp64 distances: so does the statement here)
        c = R.continuity(z, y, k, key="fp64")
        assert abs(t - manifold.trustworthiness(z.astype(np.float64), y.astype(np.float64), n_neighbors=k)) <= 1e-12
        assert abs(c - manifold.trustworthiness(y.astype(np.float64), z.astype(np.float64), n_neighbors=k)) <= 1e-12
        assert R.trustworthiness(z[:, :2], z[:, :2].copy(), k) == 1.0
    other = np.where(rng.random(lab.shape[0]) < 0.3, rng.integers(0, 8, lab.shape[0]), lab)
    for a, b, A, B in ((lab, other, 5, 8), (lab, lab, 5, 5), (lab, np.zeros_like(lab), 5, 1), (np.zeros_like(lab), np.zeros_like(lab), 1, 3),
                       (lab, rng.integers(0, 3, lab.shape[0]), 6, 3)):
        assert abs(R.nmi(a, b, A, B) - metrics.normalized_mutual_info_score(a, b)) <= 1e-12
        assert abs(R.ari(a, b, A, B) - metrics.adjusted_rand_score(a, b)) <= 1e-12


def test_the_tie_rule_and_the_self_rule():
    # five references on a line, the query at 0: distances 1, 1, 4, 0, 1 -> order by (d, j)
    r = np.array([[1.0], [-1.0], [2.0], [0.0], [1.0]], np.float32)
    q = np.array([[0.0]], np.float32)
    idx, d2 = R.search(q, r, 5)
    assert idx.tolist() == [[3, 0, 1, 4, 2]] and d2.tolist() == [[0.0, 1.0, 1.0, 1.0, 4.0]]
    assert R.ranks(q, r, np.array([[4, 2, 3, 7, -1]])).tolist() == [[3, 4, 0, -1, -1]]
    # the set against itself: self is left out, exact duplicates of self are not
    z = np.array([[0.0], [0.0], [1.0], [0.0]], np.float32)
    idx, d2 = R.search(z, z, 3, self_offset=0)
    assert idx.tolist() == [[1, 3, 2], [0, 3, 2], [0, 1, 3], [0, 1, 2]]
    assert R.ranks(z, z, np.array([[0, 1], [0, 1], [2, 3], [3, 2]]), 0).tolist() == [[-1, 0], [0, -1], [-1, 2], [-1, 2]]
    # a chunk of queries: rows 2.. of the same set with self_offset = 2
    assert np.array_equal(R.search(z[2:], z, 3, self_offset=2)[0], idx[2:])
    # a NaN reference counts as +inf and sorts last, by index; a NaN query sees every reference at +inf
    r2 = np.array([[1.0], [np.nan], [0.5], [np.nan]], np.float32)
    assert R.search(q, r2, 4)[0].tolist() == [[2, 0, 1, 3]]
    assert R.search(np.array([[np.nan]], np.float32), r2, 4)[0].tolist() == [[0, 1, 2, 3]]
    # class sums: labels outside [0, C) contribute nowhere, self stays in (sqrt(0))
    S = R.class_sums(z, z, np.array([0, 1, -1, 0]), 2)
    assert S.tolist() == [[0.0, 0.0], [0.0, 0.0], [2.0, 1.0], [0.0, 0.0]]
    # votes: ties go to the smallest label
    assert R.predict(np.array([[1, 2, 2], [0, 0, 0]])).tolist() == [1, 0]
    s, score = R.silhouette(z, np.array([0, 0, 0, 0]), 3)
    assert np.isnan(score)


# ------------------------------------------------------------------------------------------------------------- the C ABI's gates
def test_workspace_bytes_and_every_gate(L):
    lib = L.lib
    b = C.c_uint64()
    up = lambda n: (n + 255) // 256 * 256
    assert lib.gmvae_knn_workspace_bytes(100, 1000, 64, 10, 10, C.byref(b)) == 0 and b.value == up(100 * 1000 * 4)
    assert lib.gmvae_knn_workspace_bytes(7, 3, 1, 1, 256, C.byref(b)) == 0 and b.value == up(7 * 256 * 8)        # the class sums' parts are the larger
    assert lib.gmvae_knn_workspace_bytes(1, 1 << 24, 4096, 256, 256, C.byref(b)) == 0 and b.value == (1 << 24) * 4
    big = lib.gmvae_knn_workspace_bytes(1000, 60000, 64, 10, 10, C.byref(b)) == 0 and b.value
    assert big == up(1000 * 60000 * 4)                                                                            # follows Nq Nr, and nothing else
    E_NULL, E_DIMS, E_ALIGN = -1, -2, -4
    assert lib.gmvae_knn_workspace_bytes(100, 1000, 64, 10, 10, None) == E_NULL
    for bad in ((0, 10, 4, 1, 1), ((1 << 30) + 1, 10, 4, 1, 1), (4, 0, 4, 1, 1), (4, (1 << 24) + 1, 4, 1, 1), (4, 10, 0, 1, 1), (4, 10, 4097, 1, 1), (4, 10, 4, 0, 1),
                (4, 300, 4, 257, 1), (4, 10, 4, 11, 1), (4, 10, 4, 1, 0), (4, 10, 4, 1, 257)):
        assert lib.gmvae_knn_workspace_bytes(*bad, C.byref(b)) == E_DIMS, bad
    # the entry points: non-NULL, aligned host addresses that are never read -- every call below is refused before any launch
    p = lambda a=0: C.c_void_p(4096 + a)

    def search(Nq=4, Nr=10, Lz=4, k=3, so=-1, q=p(), r=p(), idx=p(), d2=p(), ws=p()):
        return lib.gmvae_knn_search(q, Nq, r, Nr, Lz, k, so, idx, d2, ws, None)

    def ranks(Nq=4, Nr=10, Lz=4, so=-1, m=3, q=p(), r=p(), cand=p(), out=p(), ws=p()):
        return lib.gmvae_knn_ranks(q, Nq, r, Nr, Lz, so, cand, m, out, ws, None)

    def sums(Nq=4, Nr=10, Lz=4, C_=3, q=p(), r=p(), lab=p(), out=p(), ws=p()):
        return lib.gmvae_knn_class_sums(q, Nq, r, Nr, Lz, lab, C_, out, ws, None)

    for fn in (search, ranks, sums):
        for kw in (dict(Nq=0), dict(Nq=(1 << 30) + 1), dict(Nr=0), dict(Nr=(1 << 24) + 1), dict(Lz=0), dict(Lz=4097)):
            assert fn(**kw) == E_DIMS, (fn.__name__, kw)
        assert fn(q=None) == E_NULL and fn(r=None) == E_NULL and fn(ws=None) == E_NULL
        assert fn(q=p(2)) == E_ALIGN and fn(ws=p(8)) == E_ALIGN
    for fn in (search, ranks):
        for kw in (dict(so=-2), dict(so=7), dict(Nq=11, Nr=10, so=0)):                   # self_offset in {-1} or [0, Nr - Nq]
            assert fn(**kw) == E_DIMS, (fn.__name__, kw)
    for kw in (dict(k=0), dict(Nr=300, k=257), dict(k=11), dict(k=10, so=0), dict(Nq=10, k=10, so=0)):
        assert search(**kw) == E_DIMS, kw
    assert search(idx=None, d2=None) == E_NULL and search(idx=p(2)) == E_ALIGN and search(d2=p(1)) == E_ALIGN
    assert ranks(m=0) == E_DIMS and ranks(m=257) == E_DIMS and ranks(cand=None) == E_NULL and ranks(out=None) == E_NULL
    assert ranks(cand=p(2)) == E_ALIGN and ranks(out=p(2)) == E_ALIGN
    assert sums(C_=0) == E_DIMS and sums(C_=257) == E_DIMS and sums(lab=None) == E_NULL and sums(out=None) == E_NULL
    assert sums(out=p(4)) == E_ALIGN and sums(lab=p(2)) == E_ALIGN
    # DIMS comes before NULL, NULL before ALIGN
    assert search(k=0, q=None) == E_DIMS and search(q=None, ws=p(8)) == E_NULL


# ------------------------------------------------------------------------------------------------------------ Python's checks
def test_python_value_errors(L, monkeypatch):
    """Everything that can be refused without touching device data is a ValueError before any tensor moves: require_gpu is stubbed
    with the CPU device, and a refused call never reaches the library."""
    import torch
    from gmvae_amd import neighbours as nb
    monkeypatch.setattr(L, "require_gpu", lambda: torch.device("cpu"))
    z, lab = torch.zeros(20, 4), torch.zeros(20, dtype=torch.int64)
    bad_calls = [
        lambda: nb.knn(torch.zeros(20), k=3), lambda: nb.knn(z, k=0), lambda: nb.knn(z, k=257), lambda: nb.knn(z, k=20),
        lambda: nb.knn(z, torch.zeros(5, 4), k=6), lambda: nb.knn(z, torch.zeros(5, 3), k=2), lambda: nb.knn(z, k=3, rows=0),
        lambda: nb.knn(z, k=3, rows=21), lambda: nb.knn(z, torch.zeros(5, 4), k=2, exclude_self=True),
        lambda: nb.knn(torch.zeros(20, 4097), k=2), lambda: nb.knn(torch.zeros(0, 4), torch.zeros(5, 4), k=2),
        lambda: nb.ranks(z, z, torch.zeros(19, 3, dtype=torch.int32)), lambda: nb.ranks(z, z, torch.zeros(20, 0, dtype=torch.int32)),
        lambda: nb.ranks(z, z, torch.zeros(20, 257, dtype=torch.int32)), lambda: nb.ranks(z, z, torch.zeros(20, 3)),
        lambda: nb.class_sums(z, z, lab, 0), lambda: nb.class_sums(z, z, lab, 257), lambda: nb.class_sums(z, z, lab[:5], 3),
        lambda: nb.class_sums(z, z, lab.float(), 3), lambda: nb.class_sums(z, z, lab, 3, rows=0),
        lambda: nb.knn_classify(z, lab, z, 3, 0), lambda: nb.knn_classify(z, lab[:3], z, 3, 4), lambda: nb.knn_accuracy_loo(z, lab, 20, 4),
        lambda: nb.silhouette(z, lab, 0), lambda: nb.silhouette(z, lab[:4], 3),
        lambda: nb.trustworthiness(z, torch.zeros(20, 2), k=10), lambda: nb.trustworthiness(z, torch.zeros(19, 2), k=2),
        lambda: nb.continuity(z, torch.zeros(20, 2), k=0),
        lambda: nb.nmi(lab, lab[:3], 2, 2), lambda: nb.ari(lab, lab, 0, 2), lambda: nb.nmi(lab.float(), lab, 2, 2),
        lambda: nb.scores(z, clusters=lab),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    assert nb.workspace_bytes(100, 1000, 64, 10, 10) == 400128
    assert nb.default_rows(60000, 60000) == (256 << 20) // 240000 and nb.default_rows(10, 60000) == 10
    # NMI and ARI are torch alone: on the CPU device they are the statement
    rng = np.random.default_rng(5)
    a, b = rng.integers(-1, 5, 300), rng.integers(0, 7, 300)
    for x, y, A, B in ((a, b, 5, 7), (a, a, 5, 5), (np.zeros(300, np.int64), np.zeros(300, np.int64), 2, 2), (a, np.zeros(300, np.int64), 5, 1)):
        assert abs(nb.nmi(torch.from_numpy(x), torch.from_numpy(y), A, B).item() - R.nmi(x, y, A, B)) <= 1e-12
        assert abs(nb.ari(torch.from_numpy(x), torch.from_numpy(y), A, B).item() - R.ari(x, y, A, B)) <= 1e-12


def test_run_gmvae_flag_checks(capsys):
    from gmvae_amd import run_gmvae
    for bad in (["--mode=eval", "--neighbour_scores=-1"], ["--mode=train", "--neighbour_scores=100"],
                ["--mode=eval", "--neighbour_scores=20", "--knn_k=10"], ["--mode=eval", "--neighbour_scores=1000", "--knn_k=257"],
                ["--mode=eval", "--neighbour_scores=1000", "--knn_k=0"]):
        with pytest.raises(SystemExit):
            cfg = run_gmvae.build_parser().parse_args(bad)
            run_gmvae.check_args(run_gmvae.build_parser(), cfg)
    capsys.readouterr()
    p = run_gmvae.build_parser()
    cfg = p.parse_args(["--mode=eval", "--neighbour_scores=21", "--knn_k=10"])
    run_gmvae.check_args(p, cfg)
    assert cfg.neighbour_scores == 21 and cfg.knn_k == 10
    assert p.parse_args([]).neighbour_scores == 0 and p.parse_args([]).knn_k == 10
