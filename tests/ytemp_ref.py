"""fp64 statement of the Gumbel GMVAE's step with the temperature as an argument and the straight-through y (include/gmvae_hip.h
GMVAE_Y_TEMP_DEV, GMVAE_Y_STRAIGHT_THROUGH), in torch with autograd -- test infrastructure, the checker of tests/test_ytemp*.py.

With g = -ln(-ln u), a_rk = (logits_bk + g_rk) / tau and y_soft = softmax_k a_rk (row r = b S + s):
    relaxed:            y = y_soft                                            (scripts/gmvae.py:238-240)
    straight-through:   y = y_soft + (y_hard - y_soft).detach(),  y_hard = e_{argmax_k (logits_bk + g_rk)} (lowest index on ties)
    log w_r = log p(x_b|z_r) + log p(z_r|y_r) - log q(z_r|x_b,y_r) - nent_b,  nent_b = sum_k q_bk ln q_bk
    L_b = -(logsumexp_s log w_bs - ln S);   at S = 1 with weights (beta_z, beta_y, 0): L_b = nll_b + beta_z kl_b + beta_y nent_b
Parameters as oracle.unpack gives them; per-net ReLU masks as oracle.loss_and_grads takes them."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O
from ymarg_ref import _mlp, _mvn_logprob


def loss_and_grads(d: O.Dims, p, x, eps, u, tau, straight_through=False, weights=None, relu_masks=None, y_leaf=False):
    """x uint8 [B, D]; eps [B S, L]; u [B S, K]; tau: the temperature (d.temperature is NOT read); weights: None or (beta_z,
    beta_y, 0) at S = 1.  y_leaf: y is the LEAF y_hard (no path back to the logits): C["dy"] = d loss / d y there, and the
    logits' gradient keeps the entropy term alone.
    Returns (C, g): C = dict(loss, nll, kl, nent -- batch means, nll and kl means over s too --, logits [B, K], dlogits [B, K] =
    d loss / d logits, y [R, K] as consumed, y_soft [R, K], argmax [R], gap [R] = the top-two gap of logits + g per row, pre =
    per-net pre-activations) and g = {name: d loss / d param} (loss = mean_b L_b), all float64 numpy."""
    rm = relu_masks or {}
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    B, K, L, S = x.shape[0], d.K, d.L, d.S
    R = B * S
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(R, L))
    ut = torch.tensor(np.asarray(u, np.float64).reshape(R, K))
    pre = {"encoder_y": [], "encoder_gmm": [], "decoder": []}
    logits = _mlp(t, "encoder_y", nl, xf, d.act, rm.get("encoder_y"), pre["encoder_y"])
    logits.retain_grad()
    lnq = torch.log_softmax(logits, dim=1)
    q = lnq.exp()
    nent = (q * lnq).sum(dim=1)
    pert = logits.repeat_interleave(S, dim=0) - torch.log(-torch.log(ut))
    y_soft = torch.softmax(pert / float(tau), dim=1)
    top2 = torch.topk(pert.detach(), 2, dim=1).values
    am = pert.detach().argmax(dim=1)                                # (the first maximal index on ties)
    y_hard = F.one_hot(am, K).to(torch.float64)
    if y_leaf:
        y = y_hard.clone().requires_grad_(True)
    elif straight_through:
        y = y_soft + (y_hard - y_soft).detach()
    else:
        y = y_soft
    xr = xf.repeat_interleave(S, dim=0)
    pp = y @ t["prior_gmm_fcnet/linear_0/w"] + t["prior_gmm_fcnet/linear_0/b"]
    qp = _mlp(t, "encoder_gmm", nl, torch.cat([xr, y], dim=1), d.act, rm.get("encoder_gmm"), pre["encoder_gmm"])
    mu_q, sig_q = qp[:, :L], torch.clamp(F.softplus(qp[:, L:] + c), min=smin)
    z = mu_q + sig_q * eps
    logq = _mvn_logprob(z, mu_q, sig_q)
    mu_p, sig_p = pp[:, :L], torch.clamp(F.softplus(pp[:, L:] + c), min=smin)
    logp = _mvn_logprob(z, mu_p, sig_p)
    lam_d = _mlp(t, "decoder", nl, z, d.act, rm.get("decoder"), pre["decoder"])
    lam_d = lam_d + torch.as_tensor(np.asarray(d.gen_bias_init, np.float64))
    logpx = (xr * lam_d - F.softplus(lam_d)).sum(dim=1)
    nll_r, kl_r = -logpx, logq - logp
    if weights is not None:
        assert S == 1 and float(weights[2]) == 0.0
        Lb = nll_r + float(weights[0]) * kl_r + float(weights[1]) * nent
    else:
        logw = (logpx + logp - logq - nent.repeat_interleave(S)).view(B, S)
        Lb = -(torch.logsumexp(logw, dim=1) - math.log(S))
    loss = Lb.mean()
    loss.backward()
    g = {k: v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy()) for k, v in t.items()}
    C = {"loss": loss.item(), "nll": nll_r.mean().item(), "kl": kl_r.mean().item(), "nent": nent.mean().item(),
         "logits": logits.detach().numpy(), "dlogits": logits.grad.numpy().copy(), "y": y.detach().numpy(),
         "y_soft": y_soft.detach().numpy(), "argmax": am.numpy(), "gap": (top2[:, 0] - top2[:, 1]).numpy(), "pre": pre,
         "dy": y.grad.numpy().copy() if y_leaf else None}
    return C, g


# ---- the shapes of tests/test_ytemp.py: the smallest that reach each branch of the head's kernels (Dims, B, seed of the inputs)
CASES = {
    "K7-S3": (O.Dims(D=100, L=5, K=7, hidden=(24, 24), S=3), 3, 42),       # R = 9: K <= 16, four rows per wave, a ragged last wave
    "K17": (O.Dims(D=64, L=8, K=17, hidden=(16,), S=1), 5, 42),            # 17 <= K <= 64: one pass
    "K65-S2": (O.Dims(D=128, L=8, K=65, hidden=(64,), S=2), 5, 42),        # K > 64: three passes (gate_corners mega-gmvae-K65's sizes)
    "K7-weights": (O.Dims(D=100, L=5, K=7, hidden=(24, 24), S=1), 8, 42),  # with GMVAE_OBJ_WEIGHTS at WEIGHTS
}
WEIGHTS = (0.25, 2.0, 0.0)
TAUS = (0.5, 2.0)
MIN_GAP = 1e-3         # every straight-through case's top-two gap of logits + g exceeds it: an fp32 argmax cannot differ from fp64's


def case_weights(name):
    return WEIGHTS if name.endswith("weights") else None


def setup(name):
    """(Dims, p as the device sees it, flat fp32, x, eps, u) of a case: Xavier parameters from seed 0, the oracle's synthetic
    inputs drawn from the case's seed."""
    d, B, seed = CASES[name]
    model = O.MODEL_GMVAE
    p = O.init_params(model, d, np.random.default_rng(0))
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    x, eps, u = O.make_inputs(d, B, model, seed_noise=seed)
    return d, p32, flat, x, eps, u
