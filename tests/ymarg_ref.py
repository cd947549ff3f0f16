"""fp64 statement of the GMVAE objective with y summed out exactly over its K values (include/gmvae_hip.h
GMVAE_OBJ_MARGINAL_Y), in torch with autograd -- test infrastructure, the checker of tests/test_ymarg*.py.

Straight from the reference's call sites with the Gumbel draw of y (scripts/gmvae.py:238-240) replaced by the enumeration:
    L_b = sum_k q(k|x_b) [ nll_bk + kl_bk ] + nent_b,   nent_b = sum_k q_bk ln q_bk  (no + ln K, as the reference)
    nll_bk = -log p(x_b | z_bk)  (gmvae.py:251-254),  kl_bk = log q(z_bk | x_b, e_k) - log p(z_bk | e_k)  (gmvae.py:243-258)
    z_bk = mu_q(x_b, e_k) + sigma_q(x_b, e_k) eps_bk  (gmvae.py:246-248)
Rows r = b*K + k.  Parameters as oracle.unpack gives them; per-net ReLU masks as oracle.loss_and_grads takes them."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O

LOG_2PI = math.log(2.0 * math.pi)


def _act(h, act):
    if act == "relu":
        return torch.relu(h)
    if act == "tanh":
        return torch.tanh(h)
    if act == "sigmoid":
        return torch.sigmoid(h)
    if act == "elu":
        return F.elu(h)
    raise ValueError(act)


def _mlp(p, name, n_layers, x, act, masks, pres):
    """snt.nets.MLP (scripts/base.py:47-60).  masks[i] (bool, optional): the ReLU subgradient of hidden layer i to take --
    the unit passes its pre-activation where the mask is set, 0 elsewhere (differs from relu only at a pre-activation that
    is zero to within rounding).  pres receives (pre-activation, sum_k |a_k| |w_kj| + |b_j|) of every hidden layer."""
    h = x
    for i in range(n_layers):
        w, b = p[f"{name}_fcnet/linear_{i}/w"], p[f"{name}_fcnet/linear_{i}/b"]
        a = h
        h = a @ w + b
        if i < n_layers - 1:
            pres.append((h.detach().numpy(), (a.abs() @ w.abs() + b.abs()).detach().numpy()))
            m = masks[i + 1] if masks is not None and i + 1 < len(masks) and masks[i + 1] is not None else None
            if m is not None:
                assert act == "relu", "subgradient masks are a ReLU matter"
                h = torch.where(torch.as_tensor(m), h, torch.zeros_like(h))
            else:
                h = _act(h, act)
    return h


def _mvn_logprob(z, mu, sigma):
    e = (z - mu) / sigma
    return (-0.5 * e * e - 0.5 * LOG_2PI).sum(dim=1) - torch.log(sigma).sum(dim=1)


def loss_and_grads(d: O.Dims, p, x, eps, relu_masks=None):
    """d: oracle.Dims (S ignored: the enumeration takes the sample axis); p: {name: array} (oracle.unpack); x uint8 [B, D];
    eps [B*K, L].  Returns (C, g): C = dict(loss, nll, kl, nent -- batch means --, logits [B,K], dlogits [B,K] = d loss /
    d logits, rows [B*K, 4] = logpx, logq, logp, log w', z [B*K, L], pre = per-net pre-activations) and g = {name: d loss /
    d param} (loss = mean_b L_b), all float64 numpy."""
    rm = relu_masks or {}
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    B, K, L, D = x.shape[0], d.K, d.L, d.D
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(B * K, L))
    pre = {"encoder_y": [], "encoder_gmm": [], "decoder": []}

    logits = _mlp(t, "encoder_y", nl, xf, d.act, rm.get("encoder_y"), pre["encoder_y"])            # gmvae.py:238
    logits.retain_grad()
    lnq = torch.log_softmax(logits, dim=1)
    q = lnq.exp()
    nent = (q * lnq).sum(dim=1)                                                                      # gmvae.py:262
    y = torch.eye(K, dtype=torch.float64).repeat(B, 1)                                               # row b K + k: e_k
    xr = xf.repeat_interleave(K, dim=0)
    pp = y @ t["prior_gmm_fcnet/linear_0/w"] + t["prior_gmm_fcnet/linear_0/b"]                       # gmvae.py:243
    qp = _mlp(t, "encoder_gmm", nl, torch.cat([xr, y], dim=1), d.act, rm.get("encoder_gmm"), pre["encoder_gmm"])  # gmvae.py:246
    mu_q, sig_q = qp[:, :L], torch.clamp(F.softplus(qp[:, L:] + c), min=smin)                        # base.py:66-72
    mu_p, sig_p = pp[:, :L], torch.clamp(F.softplus(pp[:, L:] + c), min=smin)
    z = mu_q + sig_q * eps                                                                           # gmvae.py:248
    logq = _mvn_logprob(z, mu_q, sig_q)
    logp = _mvn_logprob(z, mu_p, sig_p)                                                              # gmvae.py:258
    lam = _mlp(t, "decoder", nl, z, d.act, rm.get("decoder"), pre["decoder"])                        # gmvae.py:251
    lam = lam + torch.as_tensor(np.asarray(d.gen_bias_init, np.float64))
    logpx = (xr * lam - F.softplus(lam)).sum(dim=1)                                                  # gmvae.py:254
    lw = logpx + logp - logq                                                                         # log w' (no nent)
    qr = q.reshape(B * K)
    Lb = nent - (q * lw.view(B, K)).sum(dim=1)
    loss = Lb.mean()
    loss.backward()
    g = {k: v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy()) for k, v in t.items()}
    C = {"loss": loss.item(), "nll": (-(qr * logpx)).sum().item() / B, "kl": (qr * (logq - logp)).sum().item() / B,
         "nent": nent.mean().item(), "logits": logits.detach().numpy(), "dlogits": logits.grad.numpy(),
         "rows": torch.stack([logpx, logq, logp, lw], dim=1).detach().numpy(), "z": z.detach().numpy(), "pre": pre,
         "q": q.detach().numpy()}
    return C, g


def dlogits_closed_form(C, B):
    """d loss / d logits from the statement's own values: [ q_bj (l_bj - sum_k q_bk l_bk) + q_bj (ln q_bj - nent_b) ] / B,
    l = -log w' (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y; ymarg.hpp ymarg_rows)."""
    lg = C["logits"]
    lnq = lg - lg.max(axis=1, keepdims=True)
    lnq = lnq - np.log(np.exp(lnq).sum(axis=1, keepdims=True))
    q = np.exp(lnq)
    ell = -C["rows"][:, 3].reshape(B, -1)
    nent = (q * lnq).sum(axis=1, keepdims=True)
    return (q * (ell - (q * ell).sum(axis=1, keepdims=True)) + q * (lnq - nent)) / B
