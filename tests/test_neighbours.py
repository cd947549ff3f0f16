"""gmvae_knn_* (include/gmvae_hip.h; csrc/neigh.hpp) and gmvae_amd.neighbours on the device against the fp64 statement
(tests/neigh_ref.py): search, ranks and the classifier on a short list of sizes in three regimes -- lattice (small integers: every
distance exact in fp32, many ties; everything must equal the statement exactly), gauss and offset (N(0, 1) + 1000; the statement's
fp64 order with slack for the one rounding to fp32) --, class sums and the silhouette, trustworthiness and continuity, NaN rows,
bit-equality of two runs and of a run on a 0xFF-filled workspace, the memory contract on guarded buffers, the model and runner
surface.

The sizes sit on both sides of the kernels' constants: 256 queries a block (255, 257), 4 stored rows a block (1, 5), 32 references a
tile (2, 33), 64 lanes a row (33, 64, 65 references), 64 staged dimensions (64, 65, 130), 8 candidates a pass of the rank stage
(m = 7, 8, 9), 1024 references a slice of the class sums (1024, 1025, 4100), 16 classes held in LDS (16, 17), k up to 256."""
import math

import numpy as np
import pytest
import torch

import neigh_ref as R
from arena import Arena

pytestmark = pytest.mark.gpu

REGIMES = ["lattice", "gauss", "offset"]
REL = 2.0 ** -23          # one rounding to fp32 is 2^-24; the fp64 sum of L <= 4096 non-negative terms errs below 2^-40; 2 x for a boundary
# (Nq, Nr, L, ks, self): self = the set against itself with self excluded (Nq == Nr)
CASES = [
    (1, 2, 1, (1, 2), False),                 # k = Nr, nothing excluded
    (5, 33, 2, (1, 33), False),
    (255, 255, 7, (63,), False),
    (257, 257, 64, (64, 65), False),
    (255, 64, 65, (2, 64), False),
    (5, 4100, 130, (255, 256), False),        # a block walks several tiles per slice, and several slices
    (257, 4100, 7, (2,), False),
    (2, 2, 1, (1,), True),                    # k = Nr - 1, self excluded
    (33, 33, 2, (32,), True),
    (65, 65, 7, (63, 64), True),
    (257, 257, 64, (256,), True),
]
cid = lambda c: f"{c[0]}x{c[1]}x{c[2]}{'self' if c[4] else ''}"


def _L():
    from gmvae_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_CASE = {}


def case(c, regime):
    """(q, r, D) of a case, computed once and left unchanged."""
    key = (c, regime)
    if key not in _CASE:
        Nq, Nr, Lz, _, self_ = c
        seed = 100 * CASES.index(c) + REGIMES.index(regime) if c in CASES else 7777 + Nq + Nr + Lz
        r = R.make_codes(Nr, Lz, regime, seed)
        q = r if self_ else R.make_codes(Nq, Lz, regime, seed + 50)
        _CASE[key] = (q, r, R.dist2(q, r))
    return _CASE[key]


def candidates(Nq, Nr, m, seed):
    """Random candidates, with self (the diagonal), -1 and Nr among them."""
    cand = np.random.default_rng(seed).integers(0, Nr, (Nq, m)).astype(np.int32)
    cand[:, 0] = np.arange(Nq) % Nr
    if m > 2:
        cand[::2, 1], cand[1::2, 1] = -1, Nr
    return cand


def check_against_fp64_order(q, r, D, so, k, idx, d2):
    """The real-valued regimes: the issue's five conditions on search's output; prints the worst figures."""
    Nq, Nr = D.shape
    K, perm = R.order(q, r, so, "fp64", D)
    Ds = np.stack([K[i, p] for i, p in enumerate(perm)])                                  # the row's fp64 D in order, self left out
    ref_idx = np.stack([p[:k] for p in perm])
    e1 = np.abs(d2.astype(np.float64) - Ds[:, :k]) / Ds[:, :k]
    at = np.take_along_axis(D, idx.astype(np.int64), axis=1)
    e2 = np.abs(at - d2.astype(np.float64)) / at
    pad = np.full((Nq, 1), np.inf)
    gaps = np.diff(np.concatenate([-pad, Ds, pad], axis=1), axis=1)                       # gaps[t] = Ds[t] - Ds[t - 1]
    secure = (gaps[:, :k] > 2 * REL * Ds[:, :k]) & (gaps[:, 1:k + 1] > 2 * REL * Ds[:, :k])
    print(f"  k {k}: d2 vs t-th smallest D {e1.max():.2e}, D at idx vs d2 {e2.max():.2e} (bound {REL:.2e}); "
          f"{int(secure.sum())} of {secure.size} positions secure, {int((idx != ref_idx).sum())} differ from the fp64 order")
    assert np.isfinite(d2).all() and np.isfinite(e1).all() and np.isfinite(e2).all()
    assert e1.max() <= REL and e2.max() <= REL
    assert all(len(set(row.tolist())) == k for row in idx)
    assert np.array_equal(idx[secure], ref_idx[secure])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_search_ranks_and_votes_match_the_statement(c, regime):
    from gmvae_amd import neighbours as nb
    Nq, Nr, Lz, ks, self_ = c
    q, r, D = case(c, regime)
    so = 0 if self_ else -1
    qd, rd = dev(q), dev(r)
    labels = np.random.default_rng(5).integers(-1, 7, Nr).astype(np.int32)
    print(cid(c), regime)
    for k in ks:
        o = nb.knn(qd, None if self_ else rd, k=k)
        idx, d2 = o["idx"].cpu().numpy(), o["d2"].cpu().numpy()
        assert idx.dtype == np.int32 and idx.shape == (Nq, k) == d2.shape and idx.min() >= 0 and idx.max() < Nr
        if self_:
            assert (idx != np.arange(Nq)[:, None]).all()
        again = nb.ranks(qd, rd, o["idx"], exclude_self=self_).cpu().numpy()
        assert np.array_equal(again, np.broadcast_to(np.arange(k, dtype=np.int32), (Nq, k)))      # ranks(search) == t, exactly
        if regime == "lattice":
            ref_idx, ref_d2 = R.search(q, r, k, so, D=D)
            assert np.array_equal(idx, ref_idx) and np.array_equal(d2, ref_d2)
            cl = nb.knn_classify(rd, dev(labels), qd, k, 7, exclude_self=self_)
            v = R.votes(labels, ref_idx, 7)
            assert np.array_equal(cl["votes"].cpu().numpy(), v) and np.array_equal(cl["pred"].cpu().numpy(), R.predict(v))
        else:
            check_against_fp64_order(q, r, D, so, k, idx, d2)
    for m in sorted({1, 7, 8, 9, min(65, Nr)}):
        cand = candidates(Nq, Nr, m, 11 + m)
        got = nb.ranks(qd, rd, dev(cand), exclude_self=self_).cpu().numpy()
        if regime == "lattice":
            assert np.array_equal(got, R.ranks(q, r, cand, so, D=D)), m
        else:
            ref = R.ranks(q, r, cand, so, "fp64", D)
            slack = R.rank_slack(D, cand, so, REL)
            assert np.array_equal(got < 0, ref < 0) and (np.abs(got - ref) <= slack).all(), m
        if self_:
            assert (got[:, 0] == -1).all()                                   # the diagonal: self
        if m > 2:
            assert (got[:, 1] == -1).all()                                   # -1 and Nr: no reference


def test_chunked_queries_equal_one_call_bit_for_bit():
    """rows < N: the Python side splits the queries into several calls with self_offset > 0; every result is the one call's."""
    from gmvae_amd import neighbours as nb
    N, Lz, k = 1100, 16, 10
    for regime in REGIMES:
        z = R.make_codes(N, Lz, regime, 40)
        zd = dev(z)
        one = nb.knn(zd, k=k, rows=N)
        for rows in (1, 255, 257, 600):
            if rows == 1 and regime != "lattice":
                continue
            o = nb.knn(zd, k=k, rows=rows)
            assert torch.equal(o["idx"], one["idx"]) and torch.equal(o["d2"], one["d2"]), (regime, rows)
        if regime == "lattice":
            ref_idx, ref_d2 = R.search(z, z, k, 0)
            assert np.array_equal(one["idx"].cpu().numpy(), ref_idx) and np.array_equal(one["d2"].cpu().numpy(), ref_d2)
        cand = dev(candidates(N, N, 9, 3))
        lab = dev(np.random.default_rng(2).integers(-1, 10, N).astype(np.int32))
        rk, S = nb.ranks(zd, zd, cand, exclude_self=True, rows=N), nb.class_sums(zd, zd, lab, 10, rows=N)
        for rows in (255, 600):
            assert torch.equal(nb.ranks(zd, zd, cand, exclude_self=True, rows=rows), rk)
            assert torch.equal(nb.class_sums(zd, zd, lab, 10, rows=rows), S)
        assert torch.equal(nb.knn_accuracy_loo(zd, lab, k, 10, rows=300), nb.knn_accuracy_loo(zd, lab, k, 10))


# ------------------------------------------------------------------------------------------------- class sums and the silhouette
def labels_for(n, C, seed):
    """Random labels in [-1, C): class C - 1 empty and class C - 2 a singleton where C >= 4."""
    lab = np.random.default_rng(seed).integers(-1, C, n).astype(np.int32)
    if C >= 4:
        lab[lab >= C - 2] = 0
        lab[n // 2] = C - 2
    return lab


SUM_CASES = [(5, 33, 7, 1), (255, 257, 2, 2), (257, 1025, 64, 10), (5, 4100, 65, 65), (33, 1024, 1, 256), (257, 255, 130, 16), (5, 257, 7, 17)]


@pytest.mark.parametrize("regime", ["gauss", "offset", "lattice"])
@pytest.mark.parametrize("sc", SUM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_class_sums_match_the_statement(sc, regime):
    from gmvae_amd import neighbours as nb
    Nq, Nr, Lz, C_ = sc
    q, r, D = case((Nq, Nr, Lz, (), False), regime)
    lab = labels_for(Nr, C_, 9)
    ref = R.class_sums(q, r, lab, C_, D)
    got = nb.class_sums(dev(q), dev(r), dev(lab), C_)
    assert got.dtype == torch.float64 and got.shape == (Nq, C_)
    got = got.cpu().numpy()
    err = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    print(sc, regime, f"worst relative error {err.max():.2e} (bound 1e-11)")
    assert err.max() <= 1e-11 and np.array_equal(got == 0, ref == 0)
    if C_ >= 4:
        assert (got[:, C_ - 1] == 0).all()


@pytest.mark.parametrize("C_", [2, 10, 65, 256])
def test_silhouette_matches_the_statement(C_):
    from gmvae_amd import neighbours as nb
    N, Lz = 300, 16
    for regime in ("gauss", "offset"):
        z = R.make_codes(N, Lz, regime, 60)
        lab = labels_for(N, C_, 13)
        lab[0] = -1
        ref_s, ref_score = R.silhouette(z, lab, C_)
        o = nb.silhouette(dev(z), dev(lab), C_)
        s = o["samples"].cpu().numpy()
        assert np.array_equal(np.isnan(s), np.isnan(ref_s)) and np.isnan(s[0])
        err = np.nanmax(np.abs(s - ref_s))
        print(C_, regime, f"samples {err:.2e} (bound 1e-9), score {o['score'].item():.6f} (ref {ref_score:.6f})")
        assert err <= 1e-9 and abs(o["score"].item() - ref_score) <= 1e-9
        if C_ >= 4:
            assert s[N // 2] == 0.0                                         # the class of one: exactly 0
    one_class = np.zeros(N, np.int32)
    one_class[3] = -1
    assert math.isnan(nb.silhouette(dev(z), dev(one_class), C_)["score"].item())


@pytest.mark.parametrize("k", [1, 5, 40])
def test_trustworthiness_and_continuity(k):
    from gmvae_amd import neighbours as nb
    N, Lz = 300, 16
    x = R.make_codes(N, Lz, "gauss", 70)
    y = np.random.default_rng(71).normal(0, 1, (N, 2)).astype(np.float32)
    t, c = nb.trustworthiness(dev(x), dev(y), k), nb.continuity(dev(x), dev(y), k)
    rt, rc = R.trustworthiness(x, y, k), R.continuity(x, y, k)
    print(k, t.item(), rt, c.item(), rc)
    assert t.dtype == torch.float64 and t.dim() == 0
    assert abs(t.item() - rt) <= 1e-12 and abs(c.item() - rc) <= 1e-12
    x2 = x[:, :2].copy()
    assert nb.trustworthiness(dev(x2), dev(x2[:, :2]), k).item() == 1.0 and nb.continuity(dev(x2), dev(x2), k).item() == 1.0


def test_nan_rows():
    """One NaN row among the references and one among the queries: every index in range, the NaN reference last (by index), the
    other rows what they are without the NaN query."""
    from gmvae_amd import neighbours as nb
    Nq, Nr, Lz = 67, 255, 7
    for regime in ("lattice", "gauss"):
        r, q = R.make_codes(Nr, Lz, regime, 80), R.make_codes(Nq, Lz, regime, 81)
        r[100, 3] = np.nan
        clean = nb.knn(dev(q), dev(r), k=Nr)
        qn = q.copy()
        qn[5] = np.nan
        o = nb.knn(dev(qn), dev(r), k=Nr)
        idx, d2 = o["idx"].cpu().numpy(), o["d2"].cpu().numpy()
        assert idx.min() >= 0 and idx.max() < Nr and all(len(set(row.tolist())) == Nr for row in idx)
        keep = np.arange(Nq) != 5
        assert (idx[keep, -1] == 100).all() and np.isinf(d2[keep, -1]).all() and np.isfinite(d2[keep, :-1]).all()
        assert np.array_equal(idx[5], np.arange(Nr)) and np.isinf(d2[5]).all()
        assert np.array_equal(idx[keep], clean["idx"].cpu().numpy()[keep]) and np.array_equal(d2[keep], clean["d2"].cpu().numpy()[keep])
        if regime == "lattice":
            ref_idx, ref_d2 = R.search(qn, r, Nr)
            assert np.array_equal(idx, ref_idx) and np.array_equal(d2, ref_d2)
        cand = candidates(Nq, Nr, 9, 4)
        cand[:, 2] = 100
        rk = nb.ranks(dev(qn), dev(r), dev(cand)).cpu().numpy()
        assert (rk[keep, 2] == Nr - 1).all() and rk[5, 2] == 100             # last; for the NaN query every key ties: by index
        if regime == "lattice":
            assert np.array_equal(rk, R.ranks(qn, r, cand))
        lab = (np.arange(Nr) % 3).astype(np.int32)
        S = nb.class_sums(dev(qn), dev(r), dev(lab), 3).cpu().numpy()
        ref = R.class_sums(q, r, lab, 3)
        assert np.isnan(S[5]).all() and np.isnan(S[:, 100 % 3]).all()
        other = [c_ for c_ in range(3) if c_ != 100 % 3]
        assert np.abs(S[keep][:, other] - ref[keep][:, other]).max() <= 1e-11 * np.nanmax(ref)


# ---------------------------------------------------------------------------------------------------------------------- contract
def raw_calls(q, r, k, so, cand, lab, C_, ws):
    """Every entry point through the C ABI on the given workspace: (idx, d2, rank, sums) as arrays."""
    L = _L()
    Nq, Lz = q.shape
    Nr = r.shape[0]
    qd, rd, cd, ld = dev(q), dev(r), dev(cand), dev(lab)
    idx = torch.empty(Nq, k, dtype=torch.int32, device="cuda")
    d2 = torch.empty(Nq, k, dtype=torch.float32, device="cuda")
    rk = torch.empty(Nq, cand.shape[1], dtype=torch.int32, device="cuda")
    S = torch.empty(Nq, C_, dtype=torch.float64, device="cuda")
    st = L.current_stream()
    L.check(L.lib.gmvae_knn_search(L.ptr(qd), Nq, L.ptr(rd), Nr, Lz, k, so, L.ptr(idx), L.ptr(d2), L.ptr(ws), st), "search")
    L.check(L.lib.gmvae_knn_ranks(L.ptr(qd), Nq, L.ptr(rd), Nr, Lz, so, L.ptr(cd), cand.shape[1], L.ptr(rk), L.ptr(ws), st), "ranks")
    L.check(L.lib.gmvae_knn_class_sums(L.ptr(qd), Nq, L.ptr(rd), Nr, Lz, L.ptr(ld), C_, L.ptr(S), L.ptr(ws), st), "class_sums")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (idx, d2, rk, S))


def test_two_runs_give_the_same_bits_on_any_workspace():
    from gmvae_amd import neighbours as nb
    for (Nq, Nr, Lz, k, C_, so), regime in (((300, 1100, 64, 10, 10, -1), "gauss"), ((259, 263, 67, 65, 65, 0), "offset"),
                                            ((259, 263, 67, 65, 17, 2), "lattice")):
        r = R.make_codes(Nr, Lz, regime, 90)
        q = r[so:so + Nq] if so >= 0 else R.make_codes(Nq, Lz, regime, 91)
        cand, lab = candidates(Nq, Nr, 9, 5), labels_for(Nr, C_, 6)
        nbytes = nb.workspace_bytes(Nq, Nr, Lz, k, C_)
        a = raw_calls(q, r, k, so, cand, lab, C_, torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))
        b = raw_calls(q, r, k, so, cand, lab, C_, torch.empty(nbytes, dtype=torch.uint8, device="cuda"))
        c = raw_calls(q, r, k, so, cand, lab, C_, torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda"))
        for x, y, w in zip(a, b, c):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, w, equal_nan=True), (Nq, Nr, regime)
        assert np.isfinite(a[1]).all() and np.isfinite(a[3]).all()


def test_memory_contract_on_guarded_buffers():
    """Every entry point on arena buffers (Nq = 259, Nr = 263, L = 67, k = m = 65, C = 65: no size is a multiple of anything; then
    C = 16, the sums held in LDS): nothing changes but the named outputs and the workspace; each of search's outputs may be NULL."""
    from gmvae_amd import neighbours as nb
    L = _L()
    Nq, Nr, Lz, k, C_ = 259, 263, 67, 65, 65
    so = 3
    r = R.make_codes(Nr, Lz, "lattice", 95)
    q = r[so:so + Nq]
    D = R.dist2(q, r)
    lab = labels_for(Nr, C_, 7)
    cand = candidates(Nq, Nr, k, 8)
    ar = Arena("cuda", 24 << 20)
    f32, i32 = torch.float32, torch.int32
    bufs = {}
    for name, a, pitch, dt in (("q", q, Lz * 4, f32), ("r", r, Lz * 4, f32), ("labels", lab, 4, i32), ("cand", cand, k * 4, i32)):
        bufs[name] = ar.place(name, a.nbytes, pitch, False, dt)
        bufs[name].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    idx = ar.place("idx", Nq * k * 4, k * 4, False, i32)
    d2 = ar.place("d2", Nq * k * 4, k * 4, False, f32)
    rk = ar.place("rank", Nq * k * 4, k * 4, False, i32)
    S = ar.place("sums", Nq * C_ * 8, C_ * 8, False, torch.float64)
    ws = ar.place("workspace", nb.workspace_bytes(Nq, Nr, Lz, k, C_), 16, True, torch.uint8)
    st = L.current_stream()
    ref_idx, ref_d2 = R.search(q, r, k, so, D=D)
    for names, io, do in ((("idx", "d2"), idx, d2), (("idx",), idx, None), (("d2",), None, d2)):
        for n in ("idx", "d2"):
            ar.set_writable(n, n in names)
        ar.snapshot()
        assert L.lib.gmvae_knn_search(L.ptr(bufs["q"]), Nq, L.ptr(bufs["r"]), Nr, Lz, k, so, L.ptr(io), L.ptr(do), L.ptr(ws), st) == 0
        ar.check()
    assert np.array_equal(idx.view(Nq, k).cpu().numpy(), ref_idx) and np.array_equal(d2.view(Nq, k).cpu().numpy(), ref_d2)
    for n in ("idx", "d2"):
        ar.set_writable(n, False)
    ar.set_writable("rank", True)
    ar.snapshot()
    assert L.lib.gmvae_knn_ranks(L.ptr(bufs["q"]), Nq, L.ptr(bufs["r"]), Nr, Lz, so, L.ptr(bufs["cand"]), k, L.ptr(rk), L.ptr(ws), st) == 0
    ar.check()
    assert np.array_equal(rk.view(Nq, k).cpu().numpy(), R.ranks(q, r, cand, so, D=D))
    ar.set_writable("rank", False)
    for classes in (C_, 16):
        ar.set_writable("sums", [(0, Nq * classes * 8)])
        ar.snapshot()
        assert L.lib.gmvae_knn_class_sums(L.ptr(bufs["q"]), Nq, L.ptr(bufs["r"]), Nr, Lz, L.ptr(bufs["labels"]), classes, L.ptr(S),
                                          L.ptr(ws), st) == 0
        ar.check()
        ref = R.class_sums(q, r, lab, classes, D)
        got = S[:Nq * classes].view(Nq, classes).cpu().numpy()
        assert (np.abs(got - ref) <= 1e-11 * ref).all()


# ----------------------------------------------------------------------------------------------------------------------- surface
def reference_scores(z, labels, clusters, k, n_labels, n_clusters):
    out = {}
    if labels is not None:
        pred, _ = R.knn_classify(z, labels, z, k, n_labels, 0)
        out["knn_acc_loo"] = float((pred == labels).mean())
        out["silhouette_labels"] = R.silhouette(z, labels, n_labels)[1]
    if clusters is not None:
        out["silhouette_clusters"] = R.silhouette(z, clusters, n_clusters)[1]
        if labels is not None:
            out["nmi"], out["ari"] = R.nmi(labels, clusters, n_labels, n_clusters), R.ari(labels, clusters, n_labels, n_clusters)
    return out


def test_models_score_their_codes():
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(2)
    x = torch.from_numpy((rng.random((96, 64)) < 0.5).astype(np.uint8)).cuda()
    labels = torch.from_numpy(rng.integers(0, 4, 96)).cuda()
    given = torch.from_numpy(rng.integers(0, 5, 96)).cuda()
    plain = create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)
    gmp = create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)
    gm = create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)
    for name, model in (("vae", plain), ("vae_gmp", gmp), ("gmvae", gm)):
        z = model.transform(x).cpu().numpy()
        lab = labels.cpu().numpy()
        o = model.neighbour_scores(x, labels, k=5, n_labels=4)
        own = name != "vae"
        assert set(o) == {"knn_acc_loo", "knn_pred", "silhouette_labels", "silhouette_labels_samples"} | (
            {"silhouette_clusters", "silhouette_clusters_samples", "nmi", "ari"} if own else set()), name
        assert o["knn_pred"].shape == (96,) and o["silhouette_labels_samples"].shape == (96,) and o["knn_acc_loo"].dim() == 0
        ref = reference_scores(z, lab, None, 5, 4, None)
        for key, v in ref.items():
            assert abs(o[key].item() - v) <= 1e-9, (name, key)
        if name == "gmvae":
            cl = model.encoder_y(x).distribution.logits.argmax(dim=1).cpu().numpy()
            ref = reference_scores(z, lab, cl, 5, 4, 3)
            for key, v in ref.items():
                assert abs(o[key].item() - v) <= 1e-9, (name, key)
        o = model.neighbour_scores(x, labels, given, k=5, n_labels=4, n_clusters=5)
        ref = reference_scores(z, lab, given.cpu().numpy(), 5, 4, 5)
        for key, v in ref.items():
            assert abs(o[key].item() - v) <= 1e-9, (name, key)
        o = model.neighbour_scores(x, clusters=given, n_clusters=5)
        assert set(o) == {"silhouette_clusters", "silhouette_clusters_samples"}
    assert plain.neighbour_scores(x) == {}


def model_logits(argv, n):
    """q(y|x)'s logits of the first n examples of the split from a model restored as run_eval restores it -- built here, apart from
    the runner's own bookkeeping of batches."""
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args(argv))
    model = runners.create_model(cfg, int(getattr(cfg, "data_dim", 784)), clip=False, weighted=False, temperature_on_device=False)
    runners._restore_checkpoint(model, runners._ckpt(cfg))
    rows = [model._engine.forward(images)["logits"].clone() for images, _, _ in
            runners.create_dataset(cfg, cfg.split, shuffle=False, repeat=False, with_index=True, standardize=getattr(model, "standardize", None))]
    return torch.cat(rows)[:n]


def check_cluster_keys(res, clusters, n, k, K):
    """silhouette_clusters, nmi_clusters and ari_clusters of `res` are the module's functions on the first n codes and `clusters`."""
    from gmvae_amd import neighbours as nb
    z, lab = res["latent_state"][:n], res["labels"][:n].cuda()
    assert res["neighbour_clusters"].shape == (n,) and torch.equal(res["neighbour_clusters"], clusters)
    sil = nb.silhouette(z, clusters, K)["score"].item()
    got = res["train/silhouette_clusters"]
    assert got == sil or (math.isnan(got) and math.isnan(sil))      # (every example in one component: NaN by the statement)
    assert res["train/nmi_clusters"] == nb.nmi(lab, clusters, 10, K).item()
    assert res["train/ari_clusters"] == nb.ari(lab, clusters, 10, K).item()
    assert res[f"train/knn_acc_loo_{k}"] == nb.knn_accuracy_loo(z, lab, k, 10).item()
    assert res["train/silhouette_labels"] == nb.silhouette(z, lab, 10)["score"].item()
    return sil


def test_run_eval_reports_the_neighbour_scores(tmp_path):
    from gmvae_amd import mixfit, neighbours as nb, run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=300", "--batch_size=50"]
    run_gmvae.main(["--mode=train"] + args)
    extra = ["--fit_latent_mixture=300", "--mixture_fit_iters=5", "--embed_latent=120", "--tsne_iters=20", "--tsne_perplexity=10"]
    plain = run_gmvae.main(["--mode=eval"] + extra + args)
    # 230 of 300 examples: the scored examples end inside the fifth batch of 50
    N = 230
    res = run_gmvae.main(["--mode=eval", f"--neighbour_scores={N}", "--knn_k=7"] + extra + args)
    new = {f"train/{k}" for k in ("knn_acc_loo_7", "silhouette_labels", "silhouette_clusters", "nmi_clusters", "ari_clusters",
                                  "silhouette_latent_mixture", "nmi_latent_mixture", "ari_latent_mixture",
                                  "embedding_trustworthiness_7", "embedding_continuity_7")} | {"neighbour_clusters"}
    assert set(res) == set(plain) | new and not new & set(plain)
    for key, v in plain.items():
        if isinstance(v, float):
            assert res[key] == v, key                                           # the existing keys are unchanged
    assert torch.equal(res["latent_state"], plain["latent_state"])
    z, lab = res["latent_state"][:N], res["labels"][:N].cuda()
    clusters = model_logits(["--mode=eval"] + args, N).argmax(dim=1)
    check_cluster_keys(res, clusters, N, 7, 10)
    assigned = mixfit.assign(res["latent_state"], res["latent_mixture"])["log_resp"][:N].argmax(dim=1)
    assert res["train/silhouette_latent_mixture"] == nb.silhouette(z, assigned, 10)["score"].item()
    assert res["train/nmi_latent_mixture"] == nb.nmi(lab, assigned, 10, 10).item()
    assert res["train/ari_latent_mixture"] == nb.ari(lab, assigned, 10, 10).item()
    assert res["train/embedding_trustworthiness_7"] == nb.trustworthiness(z[:120], res["latent_embedding"], 7).item()
    assert res["train/embedding_continuity_7"] == nb.continuity(z[:120], res["latent_embedding"], 7).item()
    assert all(math.isfinite(res[k]) for k in new - {"train/silhouette_clusters", "neighbour_clusters"})
    assert 0.0 <= res["train/knn_acc_loo_7"] <= 1.0
    # the plain VAE has no clustering: the label scores alone
    vae_args = [a if not a.startswith("--model") else "--model=vae" for a in args] + [f"--logdir={tmp_path}/vae"]
    run_gmvae.main(["--mode=train"] + vae_args)
    res = run_gmvae.main(["--mode=eval", "--neighbour_scores=200", "--knn_k=3"] + vae_args)
    assert "train/knn_acc_loo_3" in res and "train/silhouette_clusters" not in res and "neighbour_clusters" not in res
    assert res["train/knn_acc_loo_3"] == nb.knn_accuracy_loo(res["latent_state"][:200], res["labels"][:200].cuda(), 3, 10).item()


def test_run_eval_scores_the_mixture_prior_vaes_posterior_clustering(tmp_path):
    """vae_gmp: the clustering is the posterior over the prior's components (--component_posterior_samples), which run_eval
    returns whole as log_posterior_component; without that flag the three cluster keys are absent."""
    from gmvae_amd import run_gmvae
    args = ["--model=vae_gmp", "--latent_size=8", "--mixture_components=4", "--max_steps=20", "--summarise_every=10",
            f"--logdir={tmp_path}", "--random_seed=1", "--synthetic_size=300", "--batch_size=50"]
    run_gmvae.main(["--mode=train"] + args)
    N = 170
    res = run_gmvae.main(["--mode=eval", f"--neighbour_scores={N}", "--knn_k=5", "--component_posterior_samples=8"] + args)
    assert res["log_posterior_component"].shape == (300, 4)
    clusters = res["log_posterior_component"][:N].argmax(dim=1)
    check_cluster_keys(res, clusters, N, 5, 4)
    assert math.isfinite(res["train/nmi_clusters"]) and math.isfinite(res["train/ari_clusters"])
    res = run_gmvae.main(["--mode=eval", f"--neighbour_scores={N}", "--knn_k=5"] + args)
    assert "train/knn_acc_loo_5" in res and not {"train/silhouette_clusters", "train/nmi_clusters", "train/ari_clusters",
                                                  "neighbour_clusters"} & set(res)
