"""fp64 statement of the GMVAE objective with y summed out exactly over its K values and z importance-weighted over S samples
per component (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y_IW), in torch with autograd -- test infrastructure, the checker of
tests/test_ymarg_iw*.py.  The networks, the Gaussian log-densities and the ReLU-mask handling are tests/objective_ref.py's:
    log w'_bsk = log p(x_b | z_bsk) + log p(z_bsk | e_k) - log q(z_bsk | x_b, e_k)
    l_bk = -( logsumexp_s log w'_bsk - ln S ),   L_b = sum_k q_bk l_bk + sum_k q_bk ln q_bk   (no + ln K, as the reference)
    z_bsk = mu_q(x_b, e_k) + sigma_q(x_b, e_k) eps_bsk
Rows r = (b*S + s)*K + k.  At S = 1 this is ymarg_ref.loss_and_grads."""
import math

import numpy as np

import objective_ref as OR
import oracle as O


def loss_and_grads(d: O.Dims, p, x, eps, S: int, relu_masks=None):
    """d: oracle.Dims (d.S ignored: S is the argument); p: {name: array} (oracle.unpack); x uint8 [B, D]; eps [B*S*K, L].
    Returns (C, g): C = dict(loss, nll, kl, nent -- batch means --, per_example [B] = L_b, logits [B,K], dlogits [B,K] =
    d loss / d logits, ell [B,K] = l_bk, q [B,K], rows [B*S*K, 4] = logpx, logq, logp, log w', z [B*S*K, L], pre =
    per-net pre-activations) and g = {name: d loss / d param} (loss = mean_b L_b), all float64 numpy."""
    c, g = OR.loss_and_grads(O.MODEL_GMVAE, d, p, x, eps, OR.summed_out, S=S, y="summed", relu_masks=relu_masks)
    nll, kl = OR.summed_means(c, c["q"])
    C = {"loss": c["loss"], "nll": nll, "kl": kl, "nent": c["nent"].mean().item(), "per_example": c["Lb"].numpy(),
         "logits": c["logits"].numpy(), "dlogits": c["dlogits"], "ell": c["ell"].numpy(), "q": c["q"].numpy(),
         "rows": OR.row_terms(c), "z": c["z"].numpy(), "pre": c["pre"]}
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
