"""fp64 statement of gmvae_simulate and gmvae_ais_reverse (include/gmvae_hip.h; csrc/bdmc.hpp): bidirectional Monte Carlo (Grosse,
Ghahramani & Adams 2015; Wu, Burda, Salakhutdinov & Grosse 2017) on the generative model of ais_ref.

  simulate: k by inverse CDF of the prior's weights with one uniform, z* = mu_k + sigma_k eps, lambda = decoder(z*) + bias,
  x_d = [ux_d < sigmoid(lambda_d)].  z* is an exact posterior sample for x.
  reverse_ais: ais_ref.ais's chain backwards.  Every chain of example b starts at z_T = z_start[b]; for t = T .. 1: one HMC
  transition on f_t (ais_ref's, draw t of the noise), then log w_rev -= (beta_t - beta_{t-1}) (B - A | B) at the new point
  z_{t-1}.  E[w_rev] = 1 / p(x): -(logsumexp_c log w_rev - ln C) is an upper bound on log p(x) in expectation.

Noise has ais_ref's layout: eps [T + 1, B C, L], u [T + 1, B C], slot 0 unused.  Target, the tables, the schedule, the margins
of the DECIDED flag and the standard error are ais_ref's own; nothing of them is restated here."""
import math

import numpy as np

import oracle as O
from oracle.gmvae_oracle import _mlp_fwd
from ais_ref import F64, STEP_MAX, STEP_MIN, Target, bound_stderr, prior_table, schedule, well_conditioned  # noqa: F401


def simulate(model, d, p, eps, u, ux):
    """eps [B, L], u [B], ux [B, D].  Returns dict(z [B, L], k [B], x [B, D] uint8, prob [B, D], pix_margin [B, D] =
    |ux - sigmoid(lambda)|, edge [B] = the distance of u to the nearest CDF edge (inf for one component))."""
    p = {k: np.asarray(v, F64) for k, v in p.items()}
    eps, u, ux = np.asarray(eps, F64), np.asarray(u, F64).reshape(-1), np.asarray(ux, F64)
    B = eps.shape[0]
    lw, mu, sg = prior_table(model, d, p)
    cdf = np.cumsum(np.exp(lw))
    K = cdf.shape[0]
    k = np.minimum((u[:, None] >= cdf[None]).sum(axis=1), K - 1)
    edge = np.abs(u[:, None] - cdf[None, :K - 1]).min(axis=1) if K > 1 else np.full(B, np.inf)
    z = mu[k] + sg[k] * eps
    lam, _ = _mlp_fwd(p, "decoder", len(d.hidden) + 1, z, act=d.act)
    prob = O.sigmoid(lam + np.asarray(d.gen_bias_init, F64))
    return dict(z=z, k=k.astype(np.int32), x=(ux < prob).astype(np.uint8), prob=prob, pix_margin=np.abs(ux - prob), edge=edge)


def reverse_ais(model, d, p, x, z_start, betas, C, n_leapfrog, step0, eps, u, init="prior", step_up=1.02, step_down=0.96, base=None):
    """The reverse chains of every example of x from z_start [B, L].  Returns dict(logw [B, C] = log w_rev, bound [B] = the upper
    bound, stats [B, 4], z [B C, L] = z_0, tail [8] (slot 0 = the sum of -bound, ais_ref's convention), accepts [T, B C] bool (row
    t - 1: transition t), decided [B C] bool, steps [B C])."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _reverse(model, d, p, x, z_start, betas, C, n_leapfrog, step0, eps, u, init, step_up, step_down, base)


def _reverse(model, d, p, x, z_start, betas, C, n_leapfrog, step0, eps, u, init, step_up, step_down, base):
    betas = np.asarray(betas, F64)
    T = len(betas) - 1
    B = np.asarray(x).shape[0]
    R = B * C
    eps = np.asarray(eps, F64).reshape(T + 1, R, d.L)
    u = np.asarray(u, F64).reshape(T + 1, R)
    tg = Target(model, d, p, x, C, init, base)
    z = np.repeat(np.asarray(z_start, F64).reshape(B, d.L), C, axis=0)
    vA, vB, gA, gB, margin = tg.parts(z)
    decided = margin > 1e-5
    logw = np.zeros(R)
    step = np.full(R, min(max(float(step0), STEP_MIN), STEP_MAX))
    accepts = np.zeros((T, R), bool)
    for t in range(T, 0, -1):
        cA, cB = tg.coef(betas[t])
        mom = eps[t].copy()
        h_old = -(cA * vA + cB * vB) + 0.5 * (mom * mom).sum(axis=1)
        e = step[:, None]
        zn = z.copy()
        mom = mom + 0.5 * e * (cA * gA + cB * gB)
        path_ok = np.ones(R, bool)
        for i in range(1, n_leapfrog + 1):
            zn = zn + e * mom
            nA, nB, ngA, ngB, margin = tg.parts(zn)
            path_ok &= margin > 1e-5
            mom = mom + (e if i < n_leapfrog else 0.5 * e) * (cA * ngA + cB * ngB)
        h_new = -(cA * nA + cB * nB) + 0.5 * (mom * mom).sum(axis=1)
        dh = h_old - h_new
        acc = np.isfinite(h_new) & (np.log(u[t]) < dh)
        decided &= path_ok & np.isfinite(h_new) & (np.abs(np.log(u[t]) - dh) > 1e-4 * (np.abs(h_old) + np.abs(h_new)) + 1e-6)
        accepts[t - 1] = acc
        a = acc[:, None]
        z, gA, gB = np.where(a, zn, z), np.where(a, ngA, gA), np.where(a, ngB, gB)
        vA, vB = np.where(acc, nA, vA), np.where(acc, nB, vB)
        step = np.clip(step * np.where(acc, step_up, step_down), STEP_MIN, STEP_MAX)
        logw = logw - (betas[t] - betas[t - 1]) * tg.dlogw(vA, vB)
    lw = logw.reshape(B, C)
    m = lw.max(axis=1, keepdims=True)
    w = np.exp(lw - m)
    bound = -(m[:, 0] + np.log(w.sum(axis=1)) - math.log(C))
    ess = w.sum(axis=1) ** 2 / (w * w).sum(axis=1)
    rate = accepts.reshape(T, B, C).mean(axis=(0, 2))
    stats = np.stack([bound, ess, rate, step.reshape(B, C).mean(axis=1)], axis=1)
    tail = np.array([-bound.sum(), ess.sum(), rate.sum(), stats[:, 3].sum(), B, 0, 0, 0], F64)
    return dict(logw=lw, bound=bound, stats=stats, z=z, tail=tail, accepts=accepts, decided=decided, steps=step)
