"""The fp64 statement of gmvae_amd.twosample (include/gmvae_hip.h gmvae_mmd; csrc/twosample.hpp): the unbiased MMD^2 of P splits of
one pooled sample, its permutation p-value and the witness function's row sums (numpy only).

    d2_ij = sum_d (z_id - z_jd)^2               (from differences, in longdouble where the platform has one)
    rbf:    k = (1/Q) sum_q exp(-gamma_q d2)    energy: k = -sqrt(d2)
    K0 = K with a zero diagonal; e = a row of E as 0 / 1, n = sum e, m = N - n
    a = e^T K0 e, b = e^T K0 1, c = 1^T K0 1
    mmd2 = a / (n (n - 1)) + (c - 2 b + a) / (m (m - 1)) - 2 (b - a) / (n m),  NaN where n < 2 or m < 2
    row_all = K0 1, row_first = K0 e_0
    p_value = (1 + #{p >= 1: mmd2[p] >= mmd2[0] - tol}) / P,  tol = 1e-8 kscale
    kscale = 1 (rbf) or the root-mean-square pairwise distance sqrt(2 N / (N - 1) sum_d var_d) (energy)
"""
import numpy as np

LD = np.longdouble
TOL = 1e-8
GATE = 1e-9          # the device's gate, in units of kscale
EDGE = 2e-9          # a split whose difference from the threshold lies within this (times kscale) is undecided


def sq_dists(z):
    """d2 [N, N] (fp64) from differences summed in longdouble."""
    z = np.asarray(z, dtype=np.float32).astype(LD)
    N = z.shape[0]
    chunk = max(1, (1 << 21) // (N * z.shape[1]))      # 2^21 differences at a time
    out = np.empty((N, N), dtype=np.float64)
    for i0 in range(0, N, chunk):
        d = z[i0:i0 + chunk, None, :] - z[None, :, :]
        out[i0:i0 + chunk] = (d * d).sum(axis=2).astype(np.float64)
    return out


def sq_dists_expanded(z):
    """The same from the expanded square n_i + n_j - 2 z_i . z_j on the rows centred by the pooled mean, in fp64 -- the form the
    statement allows a kernel for rbf."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    z = z - z.mean(axis=0)
    nrm = (z * z).sum(axis=1)
    return np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * (z @ z.T), 0.0)


def gram(d2, kernel, gamma=()):
    """K0 (fp64, zero diagonal) from d2."""
    d2 = np.asarray(d2, dtype=np.float64)
    if kernel == "energy":
        K = -np.sqrt(d2)
    elif kernel == "rbf":
        K = np.zeros_like(d2)
        for g in gamma:
            K += np.exp(-float(g) * d2)
        K /= len(gamma)
    else:
        raise ValueError(kernel)
    K = K + 0.0      # (-0.0 -> 0.0)
    np.fill_diagonal(K, 0.0)
    return K


def kscale(z, kernel):
    if kernel == "rbf":
        return 1.0
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    N = z.shape[0]
    return float(np.sqrt(2.0 * N / (N - 1) * z.var(axis=0).sum()))


def statistics(K0, E):
    """(mmd2 [P], row_all [N], row_first [N]) of the splits E [P, N]."""
    E = (np.asarray(E) != 0).astype(np.float64)
    N = K0.shape[0]
    row_all = K0.sum(axis=1)
    KE = K0 @ E.T                                    # [N, P]
    a = (E.T * KE).sum(axis=0)
    b = E @ row_all
    c = row_all.sum()
    n = E.sum(axis=1)
    m = N - n
    with np.errstate(divide="ignore", invalid="ignore"):
        out = a / (n * (n - 1)) + (c - 2 * b + a) / (m * (m - 1)) - 2 * (b - a) / (n * m)
    out[(n < 2) | (m < 2)] = np.nan
    return out, row_all, KE[:, 0].copy()


def mmd(z, E, kernel, gamma=(), d2=None):
    d2 = sq_dists(z) if d2 is None else d2
    return statistics(gram(d2, kernel, gamma), E)


def exceedances(mmd2, scale):
    """(count, undecided): the splits p >= 1 with mmd2[p] >= mmd2[0] - tol among the decided ones, and the mask [P - 1] of those
    whose difference from the threshold lies within EDGE * scale (left out of the count).  NaN splits never count."""
    diff = mmd2[1:] - (mmd2[0] - TOL * scale)
    with np.errstate(invalid="ignore"):
        undecided = np.abs(diff) <= EDGE * scale
        hit = (diff >= 0) & ~undecided
    return int(hit.sum()), undecided


def p_value(mmd2, scale):
    diff = mmd2[1:] - (mmd2[0] - TOL * scale)
    with np.errstate(invalid="ignore"):
        return (1.0 + (diff >= 0).sum()) / len(mmd2)


def witness(row_all, row_first, e0):
    e0 = (np.asarray(e0) != 0).astype(np.float64)
    N, n = len(e0), e0.sum()
    return row_first / (n - e0) - (row_all - row_first) / ((N - n) - (1 - e0))


def gammas(sigma, scales=(0.5, 1.0, 2.0)):
    return [1.0 / (2.0 * (s * sigma) ** 2) for s in scales]


def median_distance(z, rows=1024):
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    N = z.shape[0]
    sub = z[np.arange(0, N, -(-N // rows))]
    d = np.sqrt(sq_dists(sub))
    v = np.sort(d[np.triu_indices(len(sub), 1)])
    return float(v[(len(v) - 1) // 2])


def permutations(n, m, P, rng):
    N = n + m
    E = np.zeros((P, N), dtype=np.uint8)
    E[0, :n] = 1
    for p in range(1, P):
        E[p, rng.permutation(N)[:n]] = 1
    return E
