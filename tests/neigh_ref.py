"""The statement of gmvae_knn_* (include/gmvae_hip.h; csrc/neigh.hpp) and of gmvae_amd.neighbours, in NumPy fp64 -- a plain module.

Queries q [Nq, L] and references r [Nr, L] are fp32.
  Distance.  D_ij = sum_d (q_id - r_jd)^2 in the difference form, differences and sum in fp64;  d_ij = D_ij rounded once to fp32;  a
    non-finite d_ij counts as +inf.
  Order.  Reference j precedes j' for query i when (d_ij, j) < (d_ij', j') lexicographically: ties in distance go to the smaller
    index.  A total order, so nothing below depends on tiling, slicing or chunking.
  Self.  With self_offset >= 0 query i is reference row self_offset + i and is left out of the order for that query; -1: nothing is.
  Search.  idx[i, t], d2[i, t], t < k: the first k references in that order, ascending.
  Ranks.  rank[i, t] = the number of references (self left out) strictly in front of cand[i, t]; -1 for self or no reference.
  Class sums.  S[i, c] = sum over {j: labels_j = c} of sqrt(D_ij), fp64; a label outside [0, C) contributes nowhere; self stays in.
Derived: the k-NN classifier (votes, ties to the smallest label), the silhouette (scikit-learn's definition; an example whose own
label is outside [0, C) has no silhouette: NaN, and the score is the mean over the others), trustworthiness and continuity, NMI
(arithmetic normalisation) and ARI from the contingency table.
key="fp64" orders by D itself instead of d: what the tests of the real-valued regimes compare against, with slack for the rounding."""
import numpy as np


def dist2(q, r):
    """D [Nq, Nr] in fp64."""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    D = np.empty((q.shape[0], r.shape[0]), np.float64)
    block = max(1, (1 << 23) // max(1, r.shape[0] * r.shape[1]))          # (64 MiB of differences at a time)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, q.shape[0], block):
            D[a:a + block] = ((q[a:a + block, None, :] - r[None, :, :]) ** 2).sum(axis=2)
    return D


def rounded(D):
    """d: D rounded once to fp32, non-finite -> +inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = D.astype(np.float32)
    d[~np.isfinite(d)] = np.inf
    return d


def _keys(D, key):
    if key == "fp32":
        return rounded(D)
    K = D.copy()
    K[~np.isfinite(K)] = np.inf
    return K


def order(q, r, self_offset=-1, key="fp32", D=None):
    """(keys [Nq, Nr], perm): perm[i] = the references of query i in its order, self left out (a list of int arrays)."""
    D = dist2(q, r) if D is None else D
    K = _keys(D, key)
    perm = []
    for i in range(K.shape[0]):
        p = np.argsort(K[i], kind="stable")                    # stable: ties go to the smaller index
        if self_offset >= 0:
            p = p[p != self_offset + i]
        perm.append(p)
    return K, perm


def search(q, r, k, self_offset=-1, key="fp32", D=None):
    K, perm = order(q, r, self_offset, key, D)
    idx = np.stack([p[:k] for p in perm]).astype(np.int32)
    return idx, np.take_along_axis(K, idx.astype(np.int64), axis=1)


def ranks(q, r, cand, self_offset=-1, key="fp32", D=None):
    K, perm = order(q, r, self_offset, key, D)
    cand = np.asarray(cand)
    Nr = K.shape[1]
    out = np.full(cand.shape, -1, np.int32)
    for i, p in enumerate(perm):
        pos = np.full(Nr, -1, np.int64)
        pos[p] = np.arange(p.shape[0])
        ok = (cand[i] >= 0) & (cand[i] < Nr)
        out[i, ok] = pos[cand[i][ok]]
    return out


def rank_slack(D, cand, self_offset=-1, rel=2.0 ** -23):
    """Per entry: the references (self left out) whose fp64 D lies within `rel` relative of the candidate's, the candidate excluded."""
    cand = np.asarray(cand)
    out = np.zeros(cand.shape, np.int64)
    for i in range(cand.shape[0]):
        for t in range(cand.shape[1]):
            c = cand[i, t]
            if not 0 <= c < D.shape[1]:
                continue
            near = np.abs(D[i] - D[i, c]) <= rel * np.maximum(D[i], D[i, c])
            near[c] = False
            if self_offset >= 0:
                near[self_offset + i] = False
            out[i, t] = near.sum()
    return out


def class_sums(q, r, labels, C, D=None):
    D = dist2(q, r) if D is None else D
    labels = np.asarray(labels)
    with np.errstate(invalid="ignore"):
        R = np.sqrt(D)
    S = np.zeros((D.shape[0], C), np.float64)
    for c in range(C):
        S[:, c] = R[:, labels == c].sum(axis=1)
    return S


def votes(ref_labels, idx, C):
    lab = np.asarray(ref_labels)[idx]
    v = np.zeros((idx.shape[0], C), np.int64)
    for c in range(C):
        v[:, c] = (lab == c).sum(axis=1)
    return v


def predict(v):
    return v.argmax(axis=1)                                    # (NumPy's argmax returns the first maximum: the smallest label)


def knn_classify(ref, ref_labels, qry, k, C, self_offset=-1):
    v = votes(ref_labels, search(qry, ref, k, self_offset)[0], C)
    return predict(v), v


def silhouette_from_sums(S, labels, C):
    """(samples [N], score) from S [N, C] of the set against itself."""
    labels = np.asarray(labels)
    N = S.shape[0]
    valid = (labels >= 0) & (labels < C)
    n = np.bincount(labels[valid], minlength=C).astype(np.float64)
    s = np.full(N, np.nan)
    for i in range(N):
        if not valid[i]:
            continue
        ci = labels[i]
        if n[ci] == 1:
            s[i] = 0.0
            continue
        a = S[i, ci] / (n[ci] - 1)
        others = [S[i, c] / n[c] for c in range(C) if c != ci and n[c] > 0]
        b = min(others) if others else np.nan
        m = max(a, b)
        s[i] = 0.0 if m == 0 else (b - a) / m
    if (n > 0).sum() < 2:
        return s, np.nan
    return s, float(np.nanmean(s))


def silhouette(codes, labels, C):
    return silhouette_from_sums(class_sums(codes, codes, labels, C), labels, C)


def trustworthiness(X, Y, k, key="fp32"):
    """1 - 2 / (N k (2N - 3k - 1)) sum_i sum_t max(0, rank_X(i, knn_Y[i, t]) - k + 1), ranks 0-based; k < N / 2."""
    N = X.shape[0]
    assert k < N / 2
    nn_y = search(Y, Y, k, 0, key)[0]
    rk = ranks(X, X, nn_y, 0, key).astype(np.int64)
    return 1.0 - 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)) * np.maximum(rk - k + 1, 0).sum()


def continuity(X, Y, k, key="fp32"):
    return trustworthiness(Y, X, k, key)


def contingency(a, b, A, B):
    a, b = np.asarray(a), np.asarray(b)
    ok = (a >= 0) & (a < A) & (b >= 0) & (b < B)
    t = np.zeros((A, B), np.float64)
    np.add.at(t, (a[ok], b[ok]), 1.0)
    return t


def nmi(a, b, A, B):
    t = contingency(a, b, A, B)
    n = t.sum()
    ra, rb = t.sum(axis=1), t.sum(axis=0)
    if (ra > 0).sum() == 1 and (rb > 0).sum() == 1:
        return 1.0

    def ent(c):
        c = c[c > 0]
        return -(c / n * (np.log(c) - np.log(n))).sum()
    nz = t > 0
    outer = np.outer(ra, rb)
    mi = (t[nz] / n * (np.log(t[nz]) - np.log(n)) + t[nz] / n * (-np.log(outer[nz]) + 2 * np.log(n))).sum()
    h = 0.5 * (ent(ra) + ent(rb))
    return float(mi / h) if mi > 0 else 0.0


def ari(a, b, A, B):
    t = contingency(a, b, A, B)
    n = t.sum()
    sum_sq = (t ** 2).sum()
    ra, rb = (t.sum(axis=1) ** 2).sum(), (t.sum(axis=0) ** 2).sum()
    tp = sum_sq - n
    fp = rb - sum_sq
    fn = ra - sum_sq
    tn = n * n - fp - fn - sum_sq
    if fn == 0 and fp == 0:
        return 1.0
    return float(2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)))


# ------------------------------------------------------------------------------------------------------------------ test data
def make_codes(n, L, regime, seed):
    """lattice: small integers |z| <= 8 drawn from {-2..2} per dimension (many exact duplicates and equidistant points; every D is
    exact in fp32); gauss: N(0, 1); offset: N(0, 1) + 1000."""
    rng = np.random.default_rng(seed)
    if regime == "lattice":
        return rng.integers(-2, 3, (n, L)).astype(np.float32)
    z = rng.normal(0, 1, (n, L))
    if regime == "offset":
        z += 1000.0
    return z.astype(np.float32)
