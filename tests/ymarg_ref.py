"""fp64 statement of the GMVAE objective with y summed out exactly over its K values (include/gmvae_hip.h
GMVAE_OBJ_MARGINAL_Y), in torch with autograd -- test infrastructure, the checker of tests/test_ymarg*.py.

Straight from the reference's call sites with the Gumbel draw of y (scripts/gmvae.py:238-240) replaced by the enumeration:
    L_b = sum_k q(k|x_b) [ nll_bk + kl_bk ] + nent_b,   nent_b = sum_k q_bk ln q_bk  (no + ln K, as the reference)
    nll_bk = -log p(x_b | z_bk)  (gmvae.py:251-254),  kl_bk = log q(z_bk | x_b, e_k) - log p(z_bk | e_k)  (gmvae.py:243-258)
    z_bk = mu_q(x_b, e_k) + sigma_q(x_b, e_k) eps_bk  (gmvae.py:246-248)
Rows r = b*K + k.  Parameters as oracle.unpack gives them; per-net ReLU masks as oracle.loss_and_grads takes them."""
import numpy as np
import torch  # noqa: F401  (tests/saturated_cases.py reaches torch and _mlp through this module)

import objective_ref as OR
import oracle as O
from objective_ref import LOG_2PI, _act, _mlp, _mvn_logprob  # noqa: F401


def loss_and_grads(d: O.Dims, p, x, eps, relu_masks=None):
    """d: oracle.Dims (S ignored: the enumeration takes the sample axis); p: {name: array} (oracle.unpack); x uint8 [B, D];
    eps [B*K, L].  Returns (C, g): C = dict(loss, nll, kl, nent -- batch means --, logits [B,K], dlogits [B,K] = d loss /
    d logits, rows [B*K, 4] = logpx, logq, logp, log w', z [B*K, L], pre = per-net pre-activations) and g = {name: d loss /
    d param} (loss = mean_b L_b), all float64 numpy."""
    c, g = OR.loss_and_grads(O.MODEL_GMVAE, d, p, x, eps, OR.summed_out, y="summed", relu_masks=relu_masks)
    nll, kl = OR.summed_means(c, c["q"])
    C = {"loss": c["loss"], "nll": nll, "kl": kl, "nent": c["nent"].mean().item(), "logits": c["logits"].numpy(),
         "dlogits": c["dlogits"], "rows": OR.row_terms(c), "z": c["z"].numpy(), "pre": c["pre"], "q": c["q"].numpy()}
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
