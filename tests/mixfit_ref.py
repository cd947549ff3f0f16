"""The fp64 statement of gmvae_mixfit_* (include/gmvae_hip.h) and of gmvae_amd.mixfit's seeding in NumPy -- a plain module shared
by tests/test_mixfit_cpu.py and tests/test_mixfit.py.  Dense [N, K, L] arrays: it is the statement, not an implementation.  Every
function takes `dtype`, so that the same statement can be evaluated in fp32 (the yardstick for the trajectory test's tolerance).

    l_nk = logw_k - 1/2 sum_d ((z_nd - mu_kd) / sigma_kd)^2 - sum_d ln sigma_kd - (L/2) ln 2 pi
    lse_n = logsumexp_k l_nk (max-subtracted), log r_nk = l_nk - lse_n, r_nk = exp(log r_nk)
    R_k = sum_n r_nk, S1_kd = sum_n r_nk (z_nd - mu_kd), S2_kd = sum_n r_nk (z_nd - mu_kd)^2        (centred at the current mean)
    R'_k = R_k + EPS0, m = S1 / R', mu' = mu + m, sigma' = sqrt(max(S2 / R' - m^2, 0) + reg_covar), logw'_k = ln(R'_k / sum_j R'_j)
    iteration `it`: the E-step at the current parameters, loglik_history[it] = mean_n lse_n, then the M-step."""
import math

import numpy as np

EPS0 = 10 * np.finfo(np.float64).eps          # scikit-learn's constant: 10 * 2^-52


def estep(z, logw, mu, sigma, dtype=np.float64):
    """(l [N, K], lse [N], log_resp [N, K]).  A logw of -inf gives l = log_resp = -inf in that column and no NaN."""
    z, logw, mu, sigma = (np.asarray(a, dtype) for a in (z, logw, mu, sigma))
    L = z.shape[1]
    t = (z[:, None, :] - mu[None, :, :]) / sigma[None, :, :]
    with np.errstate(divide="ignore"):
        l = logw[None, :] - dtype(0.5) * (t * t).sum(axis=2) - np.log(sigma).sum(axis=1)[None, :] - dtype(0.5 * L * math.log(2 * math.pi))
    m = l.max(axis=1)
    m = np.where(np.isfinite(m), m, dtype(0))
    lse = m + np.log(np.exp(l - m[:, None]).sum(axis=1))
    return l, lse, l - lse[:, None]


def mstep(z, log_resp, mu, reg_covar, dtype=np.float64):
    """(logw', mu', sigma', R) from the responsibilities exp(log_resp), centred at the current mean `mu`."""
    z, mu = np.asarray(z, dtype), np.asarray(mu, dtype)
    r = np.exp(np.asarray(log_resp, dtype))
    dz = z[:, None, :] - mu[None, :, :]
    R = r.sum(axis=0)
    S1 = (r[:, :, None] * dz).sum(axis=0)
    S2 = (r[:, :, None] * dz * dz).sum(axis=0)
    Rp = R + dtype(EPS0)
    m = S1 / Rp[:, None]
    var = np.maximum(S2 / Rp[:, None] - m * m, dtype(0))
    return np.log(Rp / Rp.sum()), mu + m, np.sqrt(var + dtype(reg_covar)), R


def mstep_uncentred(z, log_resp, reg_covar, dtype=np.float64):
    """The restatement the kernel may NOT use: sigma'^2 = sum r z^2 / R' - mean^2 + reg_covar.  (logw', mu', sigma', R)"""
    z = np.asarray(z, dtype)
    r = np.exp(np.asarray(log_resp, dtype))
    R = r.sum(axis=0)
    Rp = R + dtype(EPS0)
    mean = (r[:, :, None] * z[:, None, :]).sum(axis=0) / Rp[:, None]
    sq = (r[:, :, None] * (z * z)[:, None, :]).sum(axis=0) / Rp[:, None]
    return np.log(Rp / Rp.sum()), mean, np.sqrt(np.maximum(sq - mean * mean, dtype(0)) + dtype(reg_covar)), R


def fit(z, logw, mu, sigma, n_iter, reg_covar=1e-6, dtype=np.float64):
    """n_iter iterations from (logw, mu, sigma): a dict of logw, mu, sigma, counts (R of the last iteration), loglik_history
    [n_iter] (the value each iteration started from), and loglik, lse and log_resp at the returned parameters."""
    logw, mu, sigma = (np.asarray(a, dtype).copy() for a in (logw, mu, sigma))
    hist, R = np.zeros(n_iter, dtype), None
    for it in range(n_iter):
        _, lse, lr = estep(z, logw, mu, sigma, dtype)
        hist[it] = lse.mean(dtype=dtype)
        logw, mu, sigma, R = mstep(z, lr, mu, reg_covar, dtype)
    _, lse, lr = estep(z, logw, mu, sigma, dtype)
    return dict(logw=logw, mu=mu, sigma=sigma, counts=R, loglik_history=hist, loglik=lse.mean(dtype=dtype), lse=lse, log_resp=lr)


def kmeanspp(z, K, u):
    """k-means++ seeding from the K uniforms u (fp32, gmvae_noise_fill's): (indices [K], margin), margin being the smallest
    distance of a threshold u_k * total from its two neighbouring cumulative sums, relative to the total (inf where no draw used a
    threshold).  i_0 = min(floor(u_0 N), N - 1); then d2min_n = the smallest squared distance (fp64 differences) to the centres so
    far, c = its cumulative sum in index order, i_k = the first index with c > u_k c[N-1]; c[N-1] = 0: i_k = min(floor(u_k N), N - 1)."""
    z, u = np.asarray(z, np.float64), np.asarray(u, np.float64)
    N = z.shape[0]
    idx = np.zeros(K, np.int64)
    idx[0] = min(int(math.floor(u[0] * N)), N - 1)
    d2 = ((z - z[idx[0]]) ** 2).sum(axis=1)
    margin = math.inf
    for k in range(1, K):
        c = np.cumsum(d2)
        if c[-1] == 0:
            idx[k] = min(int(math.floor(u[k] * N)), N - 1)
        else:
            thr = u[k] * c[-1]
            i = min(int(np.searchsorted(c, thr, side="right")), N - 1)
            idx[k] = i
            near = [abs(c[i] - thr)] + ([abs(thr - c[i - 1])] if i > 0 else [])
            margin = min(margin, min(near) / c[-1])
        d2 = np.minimum(d2, ((z - z[idx[k]]) ** 2).sum(axis=1))
    return idx, margin


def start(z, idx, reg_covar=1e-6):
    """The start of a fit from the centres `idx`: logw = -ln K, mu = the chosen rows, sigma = every component at the per-dimension
    (population) standard deviation of all codes, floored at sqrt(reg_covar)."""
    z = np.asarray(z, np.float64)
    K = len(idx)
    sd = np.maximum(z.std(axis=0), math.sqrt(reg_covar))
    return np.full(K, -math.log(K)), z[np.asarray(idx)].copy(), np.tile(sd, (K, 1))


def cluster_acc(log_resp, labels):
    """The share of points that carry their cluster's majority label (utils.cluster_acc's definition)."""
    a = np.asarray(log_resp).argmax(axis=1)
    labels = np.asarray(labels)
    return sum(np.bincount(labels[a == k]).max() for k in np.unique(a)) / len(labels)


def blobs(N, Lz, K, seed, sep=4.0, offset=0.0):
    """K clusters of unit spread, their centres `sep` apart per dimension on average and `offset` k apart in dimension 0: (codes
    as fp32 values, labels)."""
    rng = np.random.default_rng(seed)
    lab = np.arange(N) % K
    z = rng.normal(0, 1, (N, Lz)) + rng.normal(0, sep, (K, Lz))[lab]
    z[:, 0] += offset * lab
    return z.astype(np.float32), lab


def first_of_each(lab, K):
    return np.array([int(np.flatnonzero(lab == k)[0]) for k in range(K)])
