"""The fp64 statement of gmvae_mixture_logpdf_* (include/gmvae_hip.h) and of Engine.aggregate_posterior, in NumPy -- a plain
module shared by tests/test_aggpost_cpu.py and tests/test_aggpost.py.

mixture_logpdf() restates the kernel's outputs from the same fp32 arrays; components() / sample() / prior() / statement() restate
the Engine-level dict from the fp32 parameters on oracle's _mlp_fwd, _normal_head and noise, fed the Engine's own z."""
import math

import numpy as np

import oracle as O
from oracle import gmvae_oracle as OO

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def lse(a, axis):
    """logsumexp along an axis; a slice that is all -inf gives -inf (and no NaN)."""
    a = np.asarray(a, np.float64)
    m = a.max(axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m0 + np.log(np.exp(a - m0).sum(axis=axis, keepdims=True)), axis=axis)


def mixture_logpdf(z, mu, sigma, logw, log_norm=0.0, comps_per_owner=None, query_owner=None):
    """dict(log_joint [M], log_dim [M, L], log_own [M] or None) of the mixture (logw [C], mu [C, L], sigma [C, L]) at z [M, L].
    Component c belongs to example c // comps_per_owner; log_own carries no log_norm."""
    z, mu, sigma, logw = (np.asarray(a, np.float64) for a in (z, mu, sigma, logw))
    r = (z[:, None, :] - mu[None]) / sigma[None]                                   # [M, C, L]
    t = -0.5 * r * r - np.log(sigma)[None] - HALF_LOG_2PI
    s = logw[None] + t.sum(axis=2)                                                 # [M, C]
    out = dict(log_joint=lse(s, 1) - log_norm, log_dim=lse(logw[None, :, None] + t, 1) - log_norm, log_own=None)
    if query_owner is not None:
        own = (np.arange(mu.shape[0])[None] // int(comps_per_owner)) == np.asarray(query_owner)[:, None]
        out["log_own"] = lse(np.where(own, s, -np.inf), 1)
    return out


def decomposition(logpi, mu, sigma, z, qidx, prior):
    """The Engine-level dict from the components (logpi [N, Kc], mu [N, Kc, L], sigma [N, Kc, L]), the samples z [M, L] of the
    examples qidx [M] and the prior: None (standard normal) or (logw [K], mu [K, L], sigma [K, L])."""
    N, Kc, Lz = mu.shape
    z = np.asarray(z, np.float64)
    q = mixture_logpdf(z, mu.reshape(N * Kc, Lz), sigma.reshape(N * Kc, Lz), np.asarray(logpi, np.float64).reshape(-1),
                       math.log(N), Kc, qidx)
    if prior is None:
        t = -0.5 * z * z - HALF_LOG_2PI
        p = dict(log_joint=t.sum(axis=1), log_dim=t)
    else:
        p = mixture_logpdf(z, prior[1], prior[2], prior[0])
    own, agg, pri = q["log_own"], q["log_joint"], p["log_joint"]
    pi = np.exp(np.asarray(logpi, np.float64))
    ez = (pi[:, :, None] * mu).sum(axis=1)
    var = ez.var(axis=0)
    out = dict(log_q_zx=own, log_q_z=agg, log_q_zd=q["log_dim"], log_p_z=pri, log_p_zd=p["log_dim"],
               kl_avg=(own - pri).mean(), mi=(own - agg).mean(), kl_marginal=(agg - pri).mean(),
               tc=(agg - q["log_dim"].sum(axis=1)).mean(), dim_kl=(q["log_dim"] - p["log_dim"]).mean(axis=0),
               au_variance=var, active_units=int((var > 0.01).sum()))
    if Kc > 1:
        q_y = pi.mean(axis=0)
        h = lambda a: -(a * np.log(np.maximum(a, 1e-300))).sum(axis=-1)
        out.update(q_y=q_y, q_y_entropy=h(q_y), mi_xy=h(q_y) - h(pi).mean())
    return out


def _f64(p):
    return {k: np.asarray(v, np.float64) for k, v in p.items()}


def components(model, d, p, x):
    """q(z | x) as components in fp64: (logpi [N, Kc], mu [N, Kc, L], sigma [N, Kc, L]); the GMVAE's with the one-hot y."""
    p, xf = _f64(p), np.asarray(x).astype(np.float64)
    N, nl = xf.shape[0], len(d.hidden) + 1
    if model != O.MODEL_GMVAE:
        mu, sg, _ = OO._normal_head(OO._mlp_fwd(p, "encoder", nl, xf, act=d.act)[0], d.L, d.raw_sigma_bias, d.sigma_min)
        return np.zeros((N, 1)), mu[:, None, :], sg[:, None, :]
    logpi = OO._log_softmax(OO._mlp_fwd(p, "encoder_y", nl, xf, act=d.act)[0])
    xin = np.concatenate([np.repeat(xf, d.K, axis=0), np.tile(np.eye(d.K), (N, 1))], axis=1)
    mu, sg, _ = OO._normal_head(OO._mlp_fwd(p, "encoder_gmm", nl, xin, act=d.act)[0], d.L, d.raw_sigma_bias, d.sigma_min)
    return logpi, mu.reshape(N, d.K, d.L), sg.reshape(N, d.K, d.L)


def sample(model, d, comps, qidx, row0, seed, step):
    """One sample per query on oracle.noise's rows row0 + m: (z [M, L], k [M]) -- k by Gumbel-max on log pi + g."""
    logpi, mu, sg = comps
    eps, u = O.noise(len(qidx), d.L, d.K, row0, seed, step)
    k = np.zeros(len(qidx), np.int64)
    if model == O.MODEL_GMVAE:
        k = (logpi[qidx] - np.log(-np.log(u.astype(np.float64)))).argmax(axis=1)
    return mu[qidx, k] + sg[qidx, k] * eps.astype(np.float64), k


def prior(model, d, p):
    """None for the VAE's standard normal, else the prior's components (logw [K], mu [K, L], sigma [K, L])."""
    p = _f64(p)
    if model == O.MODEL_VAE:
        return None
    if model == O.MODEL_VAE_GMP:
        return OO._log_softmax(p["mixture_logits"][None])[0], p["loc"], O.softplus(p["raw_scale_diag"])
    pp = np.eye(d.K) @ p["prior_gmm_fcnet/linear_0/w"] + p["prior_gmm_fcnet/linear_0/b"]
    mu, sg, _ = OO._normal_head(pp, d.L, d.raw_sigma_bias, d.sigma_min)
    return np.full(d.K, -math.log(d.K)), mu, sg


def statement(model, d, p, x, qidx, z):
    """Engine.aggregate_posterior's dict in fp64 from the fp32 parameters p, fed the Engine's own samples z."""
    return decomposition(*components(model, d, p, x), z, np.asarray(qidx), prior(model, d, p))
