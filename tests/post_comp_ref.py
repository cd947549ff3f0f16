"""The fp64 statement of gmvae_posterior_component (include/gmvae_hip.h) from the oracle's VAE_GMP forward: per batch row b the n
copies of x_b on oracle.noise(n, L, K, (row0 + b) n, seed, step), and from its cache
    comp_sk = ln pi_k - sum_l (1/2 t_skl^2 + 1/2 ln 2 pi) - sum_l ln s_kl,      log w_sk = log p(x|z_s) + comp_sk - log q(z_s|x)
in the log domain throughout (no responsibilities)."""
import dataclasses

import numpy as np

import oracle as O

LOG_2PI = float(np.log(2.0 * np.pi))


def log_w(d, flat, x, n, row0, seed, step):
    """log w_bsk [B, n, K] in fp64."""
    p64 = O.unpack(O.MODEL_VAE_GMP, d, np.asarray(flat, np.float64))
    dn = dataclasses.replace(d, S=n)
    out = []
    for b in range(x.shape[0]):
        eps, _ = O.noise(n, d.L, d.K, (row0 + b) * n, seed, step)
        Cb = O.forward(O.MODEL_VAE_GMP, dn, p64, x[b:b + 1], eps, None)
        t, s = Cb["gmp_t"], Cb["gmp_s"]                                    # [n, K, L], [K, L]
        comp = Cb["lnw"][None] - (0.5 * t * t + 0.5 * LOG_2PI).sum(axis=2) - np.log(s).sum(axis=1)[None]
        out.append(Cb["logpx"][:, None] + comp - Cb["logq"][:, None])
    return np.array(out)


def lse(v, axis=None):
    v = np.asarray(v, np.float64)
    m = v.max(axis=axis, keepdims=True)
    return np.squeeze(m + np.log(np.exp(v - m).sum(axis=axis, keepdims=True)), axis=axis)


def log_softmax(v):
    v = np.asarray(v, np.float64)
    return v - lse(v, axis=1)[:, None]


def statement(lw):
    """From log w [B, n, K]: dict(log_joint [B, K], log_post [B, K], bound [B], ess [B]) in fp64; ESS of w_bs = sum_k w_bsk."""
    lw = np.asarray(lw, np.float64)
    lj = lse(lw, axis=1) - np.log(lw.shape[1])
    lws = lse(lw, axis=2)                                                  # [B, n]: iw_bound's own log w
    ess = np.exp(2.0 * lse(lws, axis=1) - lse(2.0 * lws, axis=1))
    return dict(log_joint=lj, log_post=log_softmax(lj), bound=lse(lj, axis=1), ess=ess)


def separate(d, flat):
    """The parameters with the mixture pulled apart: loc rows spread over +-8, raw_scale_diag = -3 (s ~ 0.05), so that for most
    components comp_k lies thousands below the mixture's logsumexp."""
    p = O.unpack(O.MODEL_VAE_GMP, d, np.asarray(flat, np.float64))
    p["loc"] = np.linspace(-8.0, 8.0, d.K)[:, None] * np.ones((1, d.L)) if d.K > 1 else np.zeros((1, d.L))
    p["raw_scale_diag"] = np.full((d.K, d.L), -3.0)
    return O.pack(O.MODEL_VAE_GMP, d, p, np.float32)
