"""fp64 statement of the semi-supervised GMVAE objective (include/gmvae_hip.h GMVAE_OBJ_LABELS, csrc/semisup.hpp), in torch with
autograd -- test infrastructure, the checker of tests/test_semisup*.py.  The networks, the Gaussian log-densities and the
ReLU-mask handling are tests/objective_ref.py's.  With l_bk = -(logsumexp_s log w'_bsk -
ln S) (at S = 1: nll_bk + kl_bk), q_b = softmax(logits_b), c_b the observed component (outside [0, K): unlabelled) and alpha
the classification weight:
    unlabelled:  L_b = sum_k q_bk l_bk + sum_k q_bk ln q_bk      (tests/ymarg_iw_ref.py's objective)
    labelled:    L_b = l_bc + alpha (-ln q_bc)                   (no entropy term; the uniform -ln p(y) left out)
Rows r = (b*S + s)*K + k.  estimator="dreg": tests/dreg_ref.py's stop-gradient statement for encoder_gmm, with the step's row
weights w_r = [k == c] softmax_s(log w'_bsc)_s for a labelled example (q_bk softmax_s for an unlabelled one) and
v_r = softmax_s(log w'_bsk)_s for every row."""
import numpy as np
import torch

import objective_ref as OR
import oracle as O


def loss_and_grads(d: O.Dims, p, x, eps, S: int, y_observed, alpha: float, relu_masks=None, estimator: str = "standard"):
    """d: oracle.Dims (d.S ignored); p: {name: array} (oracle.unpack); x uint8 [B, D]; eps [B*S*K, L]; y_observed int [B].
    Returns (C, g) as tests/ymarg_iw_ref.loss_and_grads -- C = dict(loss, nll, kl, nent -- batch means; nll / kl weigh a
    labelled example's components by [k == c] --, per_example [B], logits, dlogits, ell, q, rows, z, pre) plus ce = the sum over
    the labelled examples of -ln q_bc (not multiplied by alpha), n_labelled, hits = labelled examples with argmax_k q_bk = c_b
    (lowest index on ties), top2_gap [B] = the difference of the two largest q_bk -- and g = {name: d loss / d param}
    (loss = mean_b L_b), all float64 numpy."""
    B, K = x.shape[0], d.K
    c, g = OR.loss_and_grads(O.MODEL_GMVAE, d, p, x, eps, lambda o: OR.labelled(o, y_observed, alpha), S=S, estimator=estimator,
                             y="summed", relu_masks=relu_masks)
    qd, lab = c["q"], c["lab"]
    nll, kl = OR.summed_means(c, c["wk"])
    top2 = torch.sort(qd, dim=1, descending=True).values
    gap = (top2[:, 0] - top2[:, 1]).numpy() if K > 1 else np.ones(B)
    hits = int(((qd.argmax(dim=1) == c["c"]) & lab).sum().item())
    nent_b = torch.where(lab, torch.zeros_like(c["nent"]), c["nent"])
    C = {"loss": c["loss"], "nll": nll, "kl": kl, "nent": nent_b.mean().item(), "per_example": c["Lb"].numpy(),
         "logits": c["logits"].numpy(), "dlogits": c["dlogits"], "ell": c["ell"].numpy(), "q": qd.numpy(), "rows": OR.row_terms(c),
         "z": c["z"].numpy(), "pre": c["pre"], "ce": c["ce_b"].sum().item(), "n_labelled": int(lab.sum().item()), "hits": hits,
         "top2_gap": gap, "labelled": lab.numpy(), "w": c["w"].numpy(), "v": c["v"].numpy()}
    return C, g
