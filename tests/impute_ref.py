"""fp64 statement of gmvae_impute (include/gmvae_hip.h): imputation of the missing pixels by self-normalised importance sampling
on gmvae_iw_bound's weights (Mattei & Frellsen, MIWAE, 2019) -- test infrastructure, the checker of tests/test_impute*.py.

Built from objective_ref.forward on the regenerated noise: sample s of batch row b draws Philox row (row0 + b) n + s, its eps, the
first K columns of its u stream for the Gumbel-softmax y, and columns 4 ceil(K / 4) + m of the same stream for draw m.
    log w_bs  = lw_bs - nent_b                                  (the Gumbel objective's weight; observed pixels under a mask)
    p^_bd     = sum_s softmax_s(log w_bs) sigmoid(lam_bsd)       (every pixel)
    bound_b   = logsumexp_s log w_bs - ln n;   ESS_b = (sum w)^2 / sum w^2;   max_b = max_s softmax_s
    cond_b    = logsumexp_s (log w_bs + hid_bs) - logsumexp_s log w_bs      (0 without missing pixels)
    draw m    : s* = argmax_s (log w_bs + g_bsm), g = -ln(-ln u); ties to the lower s; z of that sample."""
import math

import numpy as np
import torch

import objective_ref as OR
import oracle as O


def u_columns(K, M):
    return 4 * ((K + 3) // 4) + M


def samples(model, d, p, x, mask, n, M, seed, step, row0=0):
    """The per-sample terms of every batch row, float64 numpy: dict(lam [B, n, D], lw [B, n] = log w, hid [B, n], z [B, n, L],
    g [B, n, M] = the draws' Gumbel noise).  x uint8 [B, D]; mask uint8 [B, D] or None (every pixel observed: hid = 0)."""
    B = x.shape[0]
    t = OR.leaves(p)
    out = dict(lam=[], lw=[], hid=[], z=[], g=[])
    for b in range(B):
        eps, u = O.noise(n, d.L, u_columns(d.K, M), (row0 + b) * n, seed, step)
        kw = dict(u=u[:, :d.K]) if model == O.MODEL_GMVAE else {}
        o = OR.forward(model, d, t, x[b:b + 1], eps, S=n, mask=None if mask is None else mask[b:b + 1], **kw)
        out["lam"].append(o["lam"].detach().numpy())
        out["lw"].append((o["lw"] - o["nent"].repeat_interleave(n)).detach().numpy())
        out["hid"].append(o["hid"].detach().numpy() if "hid" in o else np.zeros(n))
        out["z"].append(o["z"].detach().numpy())
        out["g"].append(-np.log(-np.log(u[:, u_columns(d.K, 0):].astype(np.float64))))
    return {k: np.stack(v) for k, v in out.items()}


def _lse(v, axis):
    m = v.max(axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return np.squeeze(m, axis) + np.log(np.exp(v - m).sum(axis=axis))


def estimate(lw, lam, hid=None, g=None, z=None):
    """The statement on given log weights lw [B, n] and logits lam [B, n, D] (float64): dict(mean [B, D], bound, ess, cond,
    max_weight [B], and with g [B, n, M]: draw_index [B, M], key_gap [B, M] = the best key minus the second best (inf at n = 1),
    draw_z [B, M, L] with z [B, n, L])."""
    lw = np.asarray(lw, np.float64)
    n = lw.shape[1]
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    wn = w / w.sum(axis=1, keepdims=True)
    sig = 1.0 / (1.0 + np.exp(-np.asarray(lam, np.float64)))
    o = dict(mean=np.einsum("bs,bsd->bd", wn, sig), bound=_lse(lw, 1) - math.log(n), ess=w.sum(axis=1) ** 2 / (w * w).sum(axis=1),
             max_weight=wn.max(axis=1), weights=wn)
    o["cond"] = np.zeros(lw.shape[0]) if hid is None else _lse(lw + hid, 1) - _lse(lw, 1)
    if g is not None:
        keys = lw[:, :, None] + g
        idx = keys.argmax(axis=1)                                   # (the first maximal index on ties)
        srt = np.sort(keys, axis=1)
        o["draw_index"] = idx
        o["key_gap"] = srt[:, -1] - srt[:, -2] if n > 1 else np.full(idx.shape, np.inf)
        if z is not None:
            o["draw_z"] = np.take_along_axis(z, idx[:, :, None], axis=1)
    return o


def compared_draws(lw, key_gap):
    """[B, M] bool: the draws the device test compares -- the statement's two best keys differ by more than
    2e-5 max(|log w|, 1) over the row's samples; the others are left out."""
    scale = np.maximum(np.abs(lw).max(axis=1), 1.0)
    return key_gap > 2e-5 * scale[:, None]


def mean_fp32(model, d, p, z, lw):
    """The mean image of the same statement evaluated in fp32 torch on the CPU: the decoder's layers on z [B, n, L] (rounded to
    fp32), sigmoid, softmax of the given log weights and the weighted sum, all in float32.  What rounding alone does to p^."""
    t = {k: torch.tensor(np.asarray(v, np.float32)) for k, v in p.items()}
    B, n, L = z.shape
    with torch.no_grad():
        lam = OR._mlp(t, "decoder", len(d.hidden) + 1, torch.tensor(z.reshape(B * n, L).astype(np.float32)), d.act, None, [])
        lam = lam + torch.as_tensor(np.asarray(d.gen_bias_init, np.float32))
        wn = torch.softmax(torch.tensor(np.asarray(lw, np.float32)), dim=1)
        return (wn[:, :, None] * torch.sigmoid(lam).view(B, n, -1)).sum(dim=1).numpy().astype(np.float64)


def weight_bound(g):
    """The exact bound on the change of a self-normalised sum of terms in [0, 1] when every log weight moves by at most g:
    e^{2 g} - 1."""
    return np.expm1(2.0 * np.asarray(g, np.float64))
