"""fp64 statement of the GMVAE objective with y summed out exactly over its K values and z importance-weighted over S samples
per component (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y_IW), in torch with autograd -- test infrastructure, the checker of
tests/test_ymarg_iw*.py.  The networks, the Gaussian log-densities and the ReLU-mask handling are tests/ymarg_ref.py's:
    log w'_bsk = log p(x_b | z_bsk) + log p(z_bsk | e_k) - log q(z_bsk | x_b, e_k)
    l_bk = -( logsumexp_s log w'_bsk - ln S ),   L_b = sum_k q_bk l_bk + sum_k q_bk ln q_bk   (no + ln K, as the reference)
    z_bsk = mu_q(x_b, e_k) + sigma_q(x_b, e_k) eps_bsk
Rows r = (b*S + s)*K + k.  At S = 1 this is ymarg_ref.loss_and_grads."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O
from ymarg_ref import _mlp, _mvn_logprob


def loss_and_grads(d: O.Dims, p, x, eps, S: int, relu_masks=None):
    """d: oracle.Dims (d.S ignored: S is the argument); p: {name: array} (oracle.unpack); x uint8 [B, D]; eps [B*S*K, L].
    Returns (C, g): C = dict(loss, nll, kl, nent -- batch means --, per_example [B] = L_b, logits [B,K], dlogits [B,K] =
    d loss / d logits, ell [B,K] = l_bk, q [B,K], rows [B*S*K, 4] = logpx, logq, logp, log w', z [B*S*K, L], pre =
    per-net pre-activations) and g = {name: d loss / d param} (loss = mean_b L_b), all float64 numpy."""
    rm = relu_masks or {}
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    B, K, L = x.shape[0], d.K, d.L
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(B * S * K, L))
    pre = {"encoder_y": [], "encoder_gmm": [], "decoder": []}

    logits = _mlp(t, "encoder_y", nl, xf, d.act, rm.get("encoder_y"), pre["encoder_y"])
    logits.retain_grad()
    lnq = torch.log_softmax(logits, dim=1)
    q = lnq.exp()
    nent = (q * lnq).sum(dim=1)
    y = torch.eye(K, dtype=torch.float64).repeat(B * S, 1)                                          # row (b S + s) K + k: e_k
    xr = xf.repeat_interleave(S * K, dim=0)
    pp = y @ t["prior_gmm_fcnet/linear_0/w"] + t["prior_gmm_fcnet/linear_0/b"]
    qp = _mlp(t, "encoder_gmm", nl, torch.cat([xr, y], dim=1), d.act, rm.get("encoder_gmm"), pre["encoder_gmm"])
    mu_q, sig_q = qp[:, :L], torch.clamp(F.softplus(qp[:, L:] + c), min=smin)
    mu_p, sig_p = pp[:, :L], torch.clamp(F.softplus(pp[:, L:] + c), min=smin)
    z = mu_q + sig_q * eps
    logq = _mvn_logprob(z, mu_q, sig_q)
    logp = _mvn_logprob(z, mu_p, sig_p)
    lam = _mlp(t, "decoder", nl, z, d.act, rm.get("decoder"), pre["decoder"])
    lam = lam + torch.as_tensor(np.asarray(d.gen_bias_init, np.float64))
    logpx = (xr * lam - F.softplus(lam)).sum(dim=1)
    lw = logpx + logp - logq                                                                         # log w' (no nent)
    ell = -(torch.logsumexp(lw.view(B, S, K), dim=1) - math.log(S))                                 # [B, K]
    Lb = (q * ell).sum(dim=1) + nent
    loss = Lb.mean()
    loss.backward()
    g = {k: v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy()) for k, v in t.items()}
    qd = q.detach()
    C = {"loss": loss.item(), "nll": (qd * (-logpx.detach()).view(B, S, K).mean(dim=1)).sum().item() / B,
         "kl": (qd * (logq - logp).detach().view(B, S, K).mean(dim=1)).sum().item() / B,
         "nent": nent.mean().item(), "per_example": Lb.detach().numpy(), "logits": logits.detach().numpy(),
         "dlogits": logits.grad.numpy(), "ell": ell.detach().numpy(), "q": qd.numpy(),
         "rows": torch.stack([logpx, logq, logp, lw], dim=1).detach().numpy(), "z": z.detach().numpy(), "pre": pre}
    return C, g


def enum_bounds(C, B, S, K):
    """The two outputs of gmvae_iw_bound_enum_y at n = S on the same rows: bound_b = logsumexp_{s,k} log w' - ln S and
    mean_logw_b = sum_k q_bk mean_s log w'_bsk - sum_k q_bk ln q_bk (fp64 numpy)."""
    lw = C["rows"][:, 3].reshape(B, S, K)
    m = lw.max(axis=(1, 2), keepdims=True)
    bound = (m[:, 0, 0] + np.log(np.exp(lw - m).sum(axis=(1, 2)))) - math.log(S)
    q = C["q"]
    mlw = (q * lw.mean(axis=1)).sum(axis=1) - (q * np.log(q)).sum(axis=1)
    return bound, mlw
