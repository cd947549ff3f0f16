"""fp64 statement of the doubly reparameterised gradient (Tucker et al. 2018; include/gmvae_hip.h GMVAE_GRAD_DREG) for the
importance-weighted objectives, in torch with autograd -- test infrastructure, the checker of tests/test_dreg*.py.

The estimator is stated by stop-gradients, not by its closed form.  With row weights w (the weight the step carries:
softmax_s(log w) for the VAE family, q_bk softmax_s(log w'_bsk) with y summed out, 1 at S = 1) and v = softmax_s(log w) of the
row's own sample group:
    inference parameters (`encoder` / `encoder_gmm`):  the gradient of  sum_b sum_rows (w v).detach() * (-log w_row) / B
        with log q evaluated at mu.detach(), sigma.detach() and z = mu + sigma eps left attached;
    every other parameter:  the gradient of the true loss (mean_b L_b), as tests/ymarg_iw_ref.py / the oracle state it.
estimator="standard" gives the true loss's gradient for every parameter (the plain reparameterised estimator).
The networks, the Gaussian log-density and the ReLU-mask handling are tests/ymarg_ref.py's.
Rows: VAE / VAE_GMP r = b*S + s; GMVAE (y summed out: GMVAE_OBJ_MARGINAL_Y at S = 1, GMVAE_OBJ_MARGINAL_Y_IW) r = (b*S + s)*K + k."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O
from ymarg_ref import LOG_2PI, _mlp, _mvn_logprob

INFERENCE_NET = {O.MODEL_VAE: "encoder", O.MODEL_VAE_GMP: "encoder", O.MODEL_GMVAE: "encoder_gmm"}


def is_inference(model, name):
    return name.startswith(INFERENCE_NET[model] + "_fcnet/")


def _forward(model, d, t, xf, eps, S, rm, pre, detach_q):
    """One forward pass: dict of per-row terms.  detach_q: log q at stopped (mu, sigma), z attached."""
    B, K, L = xf.shape[0], d.K, d.L
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)
    o = {}
    if model == O.MODEL_GMVAE:
        logits = _mlp(t, "encoder_y", nl, xf, d.act, rm.get("encoder_y"), pre["encoder_y"])
        logits.retain_grad()
        lnq = torch.log_softmax(logits, dim=1)
        q = lnq.exp()
        nent = (q * lnq).sum(dim=1)
        y = torch.eye(K, dtype=torch.float64).repeat(B * S, 1)
        xr = xf.repeat_interleave(S * K, dim=0)
        pp = y @ t["prior_gmm_fcnet/linear_0/w"] + t["prior_gmm_fcnet/linear_0/b"]
        qp = _mlp(t, "encoder_gmm", nl, torch.cat([xr, y], dim=1), d.act, rm.get("encoder_gmm"), pre["encoder_gmm"])
        mu_p, sig_p = pp[:, :L], torch.clamp(F.softplus(pp[:, L:] + c), min=smin)
        o.update(logits=logits, q=q, nent=nent)
    else:
        xr = xf.repeat_interleave(S, dim=0)
        qp0 = _mlp(t, "encoder", nl, xf, d.act, rm.get("encoder"), pre["encoder"])             # [B, 2L]: one row per example
        qp0.retain_grad()
        o["qp0"] = qp0
        qp = qp0.repeat_interleave(S, dim=0)
    mu_q, sig_q = qp[:, :L], torch.clamp(F.softplus(qp[:, L:] + c), min=smin)
    z = mu_q + sig_q * eps
    logq = _mvn_logprob(z, mu_q.detach(), sig_q.detach()) if detach_q else _mvn_logprob(z, mu_q, sig_q)
    if model == O.MODEL_GMVAE:
        logp = _mvn_logprob(z, mu_p, sig_p)
    elif model == O.MODEL_VAE:
        logp = (-0.5 * z * z - 0.5 * LOG_2PI).sum(dim=1)
    else:
        loc, s = t["loc"], F.softplus(t["raw_scale_diag"])
        lnw = torch.log_softmax(t["mixture_logits"], dim=0)
        tt = (z[:, None, :] - loc[None]) / s[None]
        lnN = (-0.5 * tt * tt - 0.5 * LOG_2PI).sum(dim=2) - torch.log(s).sum(dim=1)[None]
        logp = torch.logsumexp(lnw[None] + lnN, dim=1)
    lam = _mlp(t, "decoder", nl, z, d.act, rm.get("decoder"), pre["decoder"])
    lam = lam + torch.as_tensor(np.asarray(d.gen_bias_init, np.float64))
    logpx = (xr * lam - F.softplus(lam)).sum(dim=1)
    o.update(z=z, logq=logq, logp=logp, logpx=logpx, lw=logpx + logp - logq, mu_q=mu_q, sig_q=sig_q)
    return o


def _loss(model, o, B, S, K):
    """(L_b [B], v [rows] = softmax_s(log w) of the row's group, w [rows] = the step's row weight)."""
    if model == O.MODEL_GMVAE:
        lw = o["lw"].view(B, S, K)
        ell = -(torch.logsumexp(lw, dim=1) - math.log(S))
        Lb = (o["q"] * ell).sum(dim=1) + o["nent"]
        v = torch.softmax(lw, dim=1)
        w = o["q"][:, None, :] * v
        return Lb, v.reshape(-1), w.reshape(-1)
    lw = o["lw"].view(B, S)
    Lb = -(torch.logsumexp(lw, dim=1) - math.log(S))
    v = torch.softmax(lw, dim=1).reshape(-1)
    return Lb, v, v


def loss_and_grads(model: int, d: O.Dims, p, x, eps, S: int, relu_masks=None, estimator: str = "dreg"):
    """model: oracle.MODEL_*; d: oracle.Dims (d.S ignored: S is the argument); p: {name: array} (oracle.unpack); x uint8
    [B, D]; eps [rows, L].  The GMVAE is the objective with y summed out (at S = 1: GMVAE_OBJ_MARGINAL_Y).
    Returns (C, g) as tests/ymarg_iw_ref.loss_and_grads: C = dict(loss, nll, kl, nent -- batch means --, per_example [B],
    rows [rows, 4] = logpx, logq, logp, log w, z, pre; GMVAE: logits, dlogits, q; VAE family: dqp [B, 2L] = d (B loss) /
    d (the encoder's output row of example b); dmu, dsig [rows, L] = d (B loss) / d (mu_q, sigma_q) of every row) and
    g = {name: d loss / d param}, all float64 numpy."""
    assert estimator in ("standard", "dreg")
    rm = relu_masks or {}
    gm = model == O.MODEL_GMVAE
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    B, K, L = x.shape[0], d.K, d.L
    rows = B * S * (K if gm else 1)
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(rows, L))
    nets = ("encoder_y", "encoder_gmm", "decoder") if gm else ("encoder", "decoder")
    pre = {n: [] for n in nets}

    o = _forward(model, d, t, xf, eps, S, rm, pre, detach_q=False)
    o["mu_q"].retain_grad()
    o["sig_q"].retain_grad()
    Lb, v, w = _loss(model, o, B, S, K)
    loss = Lb.mean()
    loss.backward()
    g = {k: u.grad.numpy().copy() if u.grad is not None else np.zeros_like(u.detach().numpy()) for k, u in t.items()}
    dmu, dsig = o["mu_q"].grad.numpy() * B, o["sig_q"].grad.numpy() * B
    dqp = None if gm else o["qp0"].grad.numpy() * B
    dlogits = o["logits"].grad.numpy().copy() if gm else None

    if estimator == "dreg":
        t2 = {k: torch.tensor(np.asarray(u, np.float64), requires_grad=True) for k, u in p.items()}
        o2 = _forward(model, d, t2, xf, eps, S, rm, {n: [] for n in nets}, detach_q=True)
        o2["mu_q"].retain_grad()
        o2["sig_q"].retain_grad()
        sur = ((w * v).detach() * (-o2["lw"])).sum() / B
        sur.backward()
        for k in g:
            if is_inference(model, k):
                g[k] = t2[k].grad.numpy().copy()
        dmu, dsig = o2["mu_q"].grad.numpy() * B, o2["sig_q"].grad.numpy() * B
        dqp = None if gm else o2["qp0"].grad.numpy() * B

    logpx, logq, logp, lw = (o[k].detach() for k in ("logpx", "logq", "logp", "lw"))
    if gm:
        qd = o["q"].detach()
        nll = (qd * (-logpx).view(B, S, K).mean(dim=1)).sum().item() / B
        kl = (qd * (logq - logp).view(B, S, K).mean(dim=1)).sum().item() / B
        nent = o["nent"].mean().item()
    else:
        nll, kl, nent = -logpx.mean().item(), (logq - logp).mean().item(), 0.0
    C = {"loss": loss.item(), "nll": nll, "kl": kl, "nent": nent, "per_example": Lb.detach().numpy(),
         "rows": torch.stack([logpx, logq, logp, lw], dim=1).numpy(), "z": o["z"].detach().numpy(), "pre": pre,
         "dmu": dmu, "dsig": dsig, "w": w.detach().numpy(), "v": v.detach().numpy(),
         "sig_q": o["sig_q"].detach().numpy()}
    if gm:
        C.update(logits=o["logits"].detach().numpy(), dlogits=dlogits, q=o["q"].detach().numpy())
    else:
        C["dqp"] = dqp
    return C, g
