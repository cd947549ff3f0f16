"""The fp64 statement of gmvae_mixfit_full_* (include/gmvae_hip.h) in NumPy -- a plain module shared by
tests/test_mixfit_full_cpu.py and tests/test_mixfit_full.py, as tests/mixfit_ref.py is for the diagonal fit.  Every function takes
`dtype`, so that the same statement can be evaluated in fp32 (the yardstick of the trajectory test).  Parameters are logw [K],
mu [K][L] and cov [K][L][L]; only the lower triangle of cov (diagonal included) is read.

    factor: C_k = the lower Cholesky factor of that triangle, pivots p_j = a_jj - sum_{i<j} C_ji^2; a pivot that is not > 0 (NaN
            included) gives info_k = j + 1 for the first such j (LAPACK's convention), else info_k = 0
    l_nk = logw_k - 1/2 |C_k^-1 (z_n - mu_k)|^2 - sum_d ln C_k,dd - (L/2) ln 2 pi;  info_k != 0: l_nk = -inf for every n
    lse_n = logsumexp_k l_nk (max-subtracted), log r_nk = l_nk - lse_n, r_nk = exp(log r_nk)
    R_k = sum_n r_nk, S1_kd = sum_n r_nk (z_nd - mu_kd), S2_kde = sum_n r_nk (z_nd - mu_kd) (z_ne - mu_ke)    (centred at the current mean)
    R'_k = R_k + EPS0, m = S1 / R', mu' = mu + m, cov'_kde = S2_kde / R' - m_d m_e, its diagonal max(., 0) + reg_covar, written
    symmetrically; logw'_k = ln(R'_k / sum_j R'_j).  No component is special-cased: an empty or absent one keeps its mean and
    gets cov' = reg_covar I.
    iteration `it`: factor, the E-step, loglik_history[it] = mean_n lse_n, the M-step, and logw', mu', cov' ROUNDED TO FP32 (the
    ABI's parameter arrays are fp32)."""
import math

import numpy as np

from mixfit_ref import EPS0


def factor(cov, dtype=np.float64):
    """(C [K, L, L] lower triangular, info [K] int32).  Of a component with info != 0 the columns from info - 1 on are left 0."""
    cov = np.asarray(cov, dtype)
    K, L = cov.shape[0], cov.shape[1]
    C, info = np.zeros((K, L, L), dtype), np.zeros(K, np.int32)
    for k in range(K):
        a, c = cov[k], C[k]
        for j in range(L):
            p = a[j, j] - (c[j, :j] * c[j, :j]).sum(dtype=dtype)
            if not p > 0:
                info[k] = j + 1
                break
            c[j, j] = np.sqrt(p)
            c[j + 1:, j] = (a[j + 1:, j] - c[j + 1:, :j] @ c[j, :j]) / c[j, j]
    return C, info


def mahalanobis(dz, c):
    """|c^-1 dz_n|^2 [N] for lower triangular c [L, L] by forward substitution."""
    y = np.zeros_like(dz)
    for i in range(dz.shape[1]):
        y[:, i] = (dz[:, i] - y[:, :i] @ c[i, :i]) / c[i, i]
    return (y * y).sum(axis=1)


def estep(z, logw, mu, cov, dtype=np.float64):
    """(l [N, K], lse [N], log_resp [N, K], info [K]).  A logw of -inf or an info != 0 gives l = log_resp = -inf in that column
    and no NaN anywhere else."""
    z, logw, mu = (np.asarray(a, dtype) for a in (z, logw, mu))
    N, L = z.shape
    K = logw.shape[0]
    C, info = factor(cov, dtype)
    l = np.full((N, K), -np.inf, dtype)
    for k in range(K):
        if info[k] == 0:
            q = mahalanobis(z - mu[k][None, :], C[k])
            l[:, k] = logw[k] - dtype(0.5) * q - np.log(np.diagonal(C[k])).sum(dtype=dtype) - dtype(0.5 * L * math.log(2 * math.pi))
    m = l.max(axis=1)
    m = np.where(np.isfinite(m), m, dtype(0))
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    with np.errstate(invalid="ignore"):
        lr = np.where(np.isneginf(l), dtype(-np.inf), l - lse[:, None])
    return l, lse, lr, info


def mstep(z, log_resp, mu, reg_covar, dtype=np.float64):
    """(logw', mu', cov', R) from the responsibilities exp(log_resp), centred at the current mean `mu`.  A loop over k: a dense
    [N, K, L, L] array would be 340 MB at (1031, 64, 10)."""
    z, mu = np.asarray(z, dtype), np.asarray(mu, dtype)
    r = np.exp(np.asarray(log_resp, dtype))
    K, L = mu.shape
    R = r.sum(axis=0)
    Rp = R + dtype(EPS0)
    mu2, cov2 = np.zeros((K, L), dtype), np.zeros((K, L, L), dtype)
    for k in range(K):
        dz = z - mu[k][None, :]
        rd = r[:, k, None] * dz
        m = rd.sum(axis=0) / Rp[k]
        c = (rd.T @ dz) / Rp[k] - np.outer(m, m)
        c = np.tril(c) + np.tril(c, -1).T
        c[np.diag_indices(L)] = np.maximum(np.diagonal(c), dtype(0)) + dtype(reg_covar)
        mu2[k], cov2[k] = mu[k] + m, c
    return np.log(Rp / Rp.sum()), mu2, cov2, R


def fit(z, logw, mu, cov, n_iter, reg_covar=1e-6, dtype=np.float64):
    """n_iter iterations from (logw, mu, cov), the parameters rounded to fp32 after every M-step: a dict of logw, mu, cov, counts
    (R of the last iteration), loglik_history [n_iter], info [K] (a component's first non-zero value), and loglik, lse and log_resp
    at the returned parameters."""
    logw, mu, cov = (np.asarray(a, np.float32).astype(dtype) for a in (logw, mu, cov))
    hist, R, info = np.zeros(n_iter, dtype), None, np.zeros(logw.shape[0], np.int32)
    for it in range(n_iter):
        _, lse, lr, inf_it = estep(z, logw, mu, cov, dtype)
        info = inf_it if it == 0 else np.where(info == 0, inf_it, info)
        hist[it] = lse.mean(dtype=dtype)
        logw, mu, cov, R = (a.astype(np.float32).astype(dtype) if i < 3 else a for i, a in enumerate(mstep(z, lr, mu, reg_covar, dtype)))
    _, lse, lr, _ = estep(z, logw, mu, cov, dtype)
    return dict(logw=logw, mu=mu, cov=cov, counts=R, loglik_history=hist, info=info, loglik=lse.mean(dtype=dtype), lse=lse, log_resp=lr)


def start(z, idx, reg_covar=1e-6):
    """The start of a full fit from the centres `idx`: mixfit_ref.start's logw and mu, cov_k = diag(sd^2) of all codes floored at
    reg_covar -- so the first E-step is the diagonal fit's."""
    z = np.asarray(z, np.float64)
    K = len(idx)
    var = np.maximum(z.var(axis=0), reg_covar)
    return np.full(K, -math.log(K)), z[np.asarray(idx)].copy(), np.tile(np.diag(var), (K, 1, 1))


def stripes(N, L, K, seed, gap, length):
    """K parallel elongated clusters: z ~ N(0, I), stretched to spread `length` along u = (1, 1, 0, ...) / sqrt 2, shifted by gap
    (n mod K) along v = (1, -1, 0, ...) / sqrt 2: (codes as fp32 values, labels)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 1, (N, L))
    u, v = np.zeros(L), np.zeros(L)
    u[:2] = 1 / math.sqrt(2)
    v[0], v[1] = 1 / math.sqrt(2), -1 / math.sqrt(2)
    z += (length - 1) * (z @ u)[:, None] * u[None, :]
    lab = np.arange(N) % K
    z += gap * lab[:, None] * v[None, :]
    return z.astype(np.float32), lab


def n_parameters(K, L, covariance):
    """scikit-learn's GaussianMixture._n_parameters."""
    return K - 1 + K * L + (K * L * (L + 1) // 2 if covariance == "full" else K * L)
