"""The fp64 statement of gmvae_pca_* and gmvae_sym_eigh (include/gmvae_hip.h; csrc/pca.hpp) in NumPy: the mean and the centred
covariance, the eigendecomposition with the library's ordering and sign rule, the subspace iteration exactly as the library runs
it, transform, whitening, the Frechet distance -- and the round-robin Jacobi sweep, restated only to choose the default number of
sweeps (tests/test_pca_cpu.py; profiles/pca_notes.md).  No GPU, no torch."""
import numpy as np

MAX_DENSE = 128      # the library's gate: up to here the solver runs on C itself, and m = D


def moments(x):
    """mu [D], C [D, D] = sum (x - mu)(x - mu)^T / (N - 1): centred before the product."""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=0)
    xc = x - mu
    return mu, xc.T @ xc / (x.shape[0] - 1)


def sign_rows(comp):
    """Each row signed so that its entry of largest magnitude (the first such index) is positive."""
    comp = np.array(comp, dtype=np.float64)
    for r in comp:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1.0
    return comp


def eigh(A):
    """(w descending, V with the eigenvectors in its columns, signed by the rule); the lower triangle of A is read."""
    w, V = np.linalg.eigh(np.asarray(A, dtype=np.float64), UPLO="L")
    order = np.argsort(-w, kind="stable")
    return w[order], sign_rows(V[:, order].T).T


def cholesky(G):
    """(R lower with G = R R^T, info): info = 0, or 1 + the first pivot that is not > 0 (R is then unfinished) -- the rule of
    mff_factor_lds (csrc/mixfit_common.hpp)."""
    a = np.array(G, dtype=np.float64)
    n = a.shape[0]
    for t in range(n):
        p = a[t, t]
        if not p > 0.0:
            return np.tril(a), t + 1
        c = np.sqrt(p)
        a[t + 1:, t] /= c
        a[t, t] = c
        a[t + 1:, t + 1:] -= np.outer(a[t + 1:, t], a[t + 1:, t])
    return np.tril(a), 0


def subspace(C, V0, n_iter):
    """n_iter times W = C V, G = W^T W = R R^T, V = W R^-T; then W = C V, T = (V^T W + W^T V) / 2 = Q diag(theta) Q^T.
    (theta, components [m, D] signed, residual [m], info)."""
    V = np.array(V0, dtype=np.float64)
    m = V.shape[1]
    for _ in range(n_iter):
        W = C @ V
        R, info = cholesky(W.T @ W)
        if info:
            return None, None, None, info
        V = W @ np.linalg.inv(R).T
    W = C @ V
    T = V.T @ W
    theta, Q = eigh(0.5 * (T + T.T))
    Y, Z = V @ Q, W @ Q
    return theta, sign_rows(Y.T), np.sqrt(((Z - Y * theta) ** 2).sum(axis=0)), 0


def start(D, m, seed=0):
    """The orthonormal start a caller without torch uses in the tests: QR of fp64 normals."""
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((D, m)))[0]


def fit(x, k=None, m=None, n_iter=0, V0=None):
    """The dict gmvae_amd.pca.fit returns (offdiag aside), from the statement."""
    x = np.asarray(x)
    N, D = x.shape
    mu, C = moments(x)
    k = min(D, MAX_DENSE) if k is None else k
    out = {"mean": mu, "total_variance": np.trace(C), "covariance": C, "info": 0}
    if D <= MAX_DENSE:
        w, V = eigh(C)
        comp, var, res = V.T[:k], w[:k], np.zeros(k)
    else:
        theta, Y, r, info = subspace(C, V0, n_iter)
        if info:
            nan = np.full(k, np.nan)
            out.update(info=info, components=np.full((k, D), np.nan), explained_variance=nan, explained_variance_ratio=nan, residual=nan)
            return out
        comp, var, res = Y[:k], theta[:k], r[:k]
    out.update(components=comp, explained_variance=var, explained_variance_ratio=var / out["total_variance"], residual=res)
    return out


def transform(x, fitted, whiten=False):
    z = (np.asarray(x, dtype=np.float64) - fitted["mean"]) @ fitted["components"].T
    if whiten:
        v = fitted["explained_variance"]
        z = z * np.where(v > 0, 1.0 / np.sqrt(np.where(v > 0, v, 1.0)), 0.0)
    return z


def inverse_transform(z, fitted):
    return np.asarray(z, dtype=np.float64) @ fitted["components"] + fitted["mean"]


def spectrum_summary(var, total):
    ratio = var / total
    return {"dim90": int(np.searchsorted(np.cumsum(ratio), 0.9) + 1), "participation": var.sum() ** 2 / (var ** 2).sum(),
            "top_ratio": ratio[0]}


def frechet(x, y):
    """|mu1 - mu2|^2 + tr C1 + tr C2 - 2 sum sqrt(max(beta, 0)), beta the eigenvalues of S^1/2 U^T C2 U S^1/2 with C1 = U S U^T.
    (distance, mean part, covariance part)."""
    m1, C1 = moments(x)
    m2, C2 = moments(y)
    s, U = eigh(C1)
    h = np.sqrt(np.maximum(s, 0.0))
    M = (U * h).T @ C2 @ (U * h)
    beta = np.linalg.eigvalsh(0.5 * (M + M.T))
    mean_part = ((m1 - m2) ** 2).sum()
    cov_part = np.trace(C1) + np.trace(C2) - 2.0 * np.sqrt(np.maximum(beta, 0.0)).sum()
    return mean_part + cov_part, mean_part, cov_part


def round_robin(n, r):
    """The pairs (p < q) of round r of a sweep, as csrc/pca.hpp forms them: with ne = n rounded up to even, (ne - 1, r) and
    ((r + k) mod (ne - 1), (r - k) mod (ne - 1)) for k = 1 .. ne / 2 - 1; a pair holding an index >= n (the bye) is left out."""
    ne = (n + 1) & ~1
    ring = ne - 1
    k = np.arange(1, ne // 2)
    u = np.concatenate(([ne - 1], (r + k) % ring))
    v = np.concatenate(([r], (r - k) % ring))
    p, q = np.minimum(u, v), np.maximum(u, v)
    keep = q < n
    return p[keep], q[keep]


def jacobi(A, n_sweeps):
    """Cyclic Jacobi in the library's round-robin ordering and with its rotation: (w, V, offdiag) UNSORTED -- used to choose the
    default n_sweeps and to show the ordering converges; the tests compare the device with `eigh` above."""
    a = np.array(A, dtype=np.float64)
    a = np.tril(a) + np.tril(a, -1).T
    n = a.shape[0]
    V = np.eye(n)
    ne = (n + 1) & ~1
    for _ in range(n_sweeps):
        for r in range(ne - 1):
            p, q = round_robin(n, r)
            apq = a[q, p]
            on = apq != 0.0
            p, q, apq = p[on], q[on], apq[on]
            if len(p) == 0:
                continue
            with np.errstate(over="ignore"):
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            app, aqq = a[p, p] - t * apq, a[q, q] + t * apq
            rp, rq = a[p, :].copy(), a[q, :].copy()
            a[p, :], a[q, :] = c[:, None] * rp - s[:, None] * rq, s[:, None] * rp + c[:, None] * rq
            cp, cq = a[:, p].copy(), a[:, q].copy()
            a[:, p], a[:, q] = c * cp - s * cq, s * cp + c * cq
            a[p, p], a[q, q], a[p, q], a[q, p] = app, aqq, 0.0, 0.0
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
    return np.diag(a).copy(), V, offdiag(a)


def offdiag(a):
    dia = np.abs(np.diag(a)).max()
    return np.abs(a - np.diag(np.diag(a))).max() / dia if dia > 0 else 0.0


def fixture(N, D, decay=0.9, seed=0, offset=1.0, rank=None):
    """N fp32 rows = normals . sqrt(decay^j) in a random orthogonal basis (the first `rank` directions only), plus an offset vector."""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((D, D)))[0]
    sd = np.sqrt(decay ** np.arange(D))
    if rank is not None:
        sd[rank:] = 0.0
    z = rng.standard_normal((N, D)) * sd
    return (z @ basis.T + offset * rng.standard_normal(D)).astype(np.float32)
