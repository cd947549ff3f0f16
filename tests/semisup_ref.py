"""fp64 statement of the semi-supervised GMVAE objective (include/gmvae_hip.h GMVAE_OBJ_LABELS, csrc/semisup.hpp), in torch with
autograd -- test infrastructure, the checker of tests/test_semisup*.py.  The networks, the Gaussian log-densities and the
ReLU-mask handling are tests/ymarg_ref.py's (through tests/dreg_ref.py's forward pass).  With l_bk = -(logsumexp_s log w'_bsk -
ln S) (at S = 1: nll_bk + kl_bk), q_b = softmax(logits_b), c_b the observed component (outside [0, K): unlabelled) and alpha
the classification weight:
    unlabelled:  L_b = sum_k q_bk l_bk + sum_k q_bk ln q_bk      (tests/ymarg_iw_ref.py's objective)
    labelled:    L_b = l_bc + alpha (-ln q_bc)                   (no entropy term; the uniform -ln p(y) left out)
Rows r = (b*S + s)*K + k.  estimator="dreg": tests/dreg_ref.py's stop-gradient statement for encoder_gmm, with the step's row
weights w_r = [k == c] softmax_s(log w'_bsc)_s for a labelled example (q_bk softmax_s for an unlabelled one) and
v_r = softmax_s(log w'_bsk)_s for every row."""
import math

import numpy as np
import torch

import oracle as O
from dreg_ref import _forward, is_inference


def loss_and_grads(d: O.Dims, p, x, eps, S: int, y_observed, alpha: float, relu_masks=None, estimator: str = "standard"):
    """d: oracle.Dims (d.S ignored); p: {name: array} (oracle.unpack); x uint8 [B, D]; eps [B*S*K, L]; y_observed int [B].
    Returns (C, g) as tests/ymarg_iw_ref.loss_and_grads -- C = dict(loss, nll, kl, nent -- batch means; nll / kl weigh a
    labelled example's components by [k == c] --, per_example [B], logits, dlogits, ell, q, rows, z, pre) plus ce = the sum over
    the labelled examples of -ln q_bc (not multiplied by alpha), n_labelled, hits = labelled examples with argmax_k q_bk = c_b
    (lowest index on ties), top2_gap [B] = the difference of the two largest q_bk -- and g = {name: d loss / d param}
    (loss = mean_b L_b), all float64 numpy."""
    assert estimator in ("standard", "dreg")
    rm = relu_masks or {}
    model = O.MODEL_GMVAE
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    B, K, L = x.shape[0], d.K, d.L
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(B * S * K, L))
    c = torch.as_tensor(np.asarray(y_observed).astype(np.int64).reshape(B))
    lab = (c >= 0) & (c < K)
    cc = torch.where(lab, c, torch.zeros_like(c))
    onehot = torch.nn.functional.one_hot(cc, K).double() * lab[:, None].double()          # zero rows where unlabelled
    nets = ("encoder_y", "encoder_gmm", "decoder")
    pre = {n: [] for n in nets}

    o = _forward(model, d, t, xf, eps, S, rm, pre, detach_q=False)
    lnq = torch.log_softmax(o["logits"], dim=1)
    q = o["q"]
    lw = o["lw"].view(B, S, K)
    ell = -(torch.logsumexp(lw, dim=1) - math.log(S))
    ce_b = -(onehot * lnq).sum(dim=1)                                                       # 0 where unlabelled
    L_unl = (q * ell).sum(dim=1) + o["nent"]
    L_lab = (onehot * ell).sum(dim=1) + alpha * ce_b
    Lb = torch.where(lab, L_lab, L_unl)
    loss = Lb.mean()
    loss.backward()
    g = {k: u.grad.numpy().copy() if u.grad is not None else np.zeros_like(u.detach().numpy()) for k, u in t.items()}
    dlogits = o["logits"].grad.numpy().copy()
    wk = torch.where(lab[:, None], onehot, q.detach())                                      # the component weights [B, K]
    v = torch.softmax(lw.detach(), dim=1)
    w = (wk[:, None, :] * v).reshape(-1)

    if estimator == "dreg":
        t2 = {k: torch.tensor(np.asarray(u, np.float64), requires_grad=True) for k, u in p.items()}
        o2 = _forward(model, d, t2, xf, eps, S, rm, {n: [] for n in nets}, detach_q=True)
        sur = ((w * v.reshape(-1)).detach() * (-o2["lw"])).sum() / B
        sur.backward()
        for k in g:
            if is_inference(model, k):
                g[k] = t2[k].grad.numpy().copy()

    logpx, logq, logp = (o[k].detach() for k in ("logpx", "logq", "logp"))
    qd = q.detach()
    top2 = torch.sort(qd, dim=1, descending=True).values
    gap = (top2[:, 0] - top2[:, 1]).numpy() if K > 1 else np.ones(B)
    hits = int(((qd.argmax(dim=1) == c) & lab).sum().item())
    nent_b = torch.where(lab, torch.zeros_like(o["nent"]), o["nent"]).detach()
    C = {"loss": loss.item(), "nll": (wk * (-logpx).view(B, S, K).mean(dim=1)).sum().item() / B,
         "kl": (wk * (logq - logp).view(B, S, K).mean(dim=1)).sum().item() / B, "nent": nent_b.mean().item(),
         "per_example": Lb.detach().numpy(), "logits": o["logits"].detach().numpy(), "dlogits": dlogits,
         "ell": ell.detach().numpy(), "q": qd.numpy(),
         "rows": torch.stack([logpx, logq, logp, o["lw"].detach()], dim=1).numpy(), "z": o["z"].detach().numpy(), "pre": pre,
         "ce": ce_b.detach().sum().item(), "n_labelled": int(lab.sum().item()), "hits": hits, "top2_gap": gap,
         "labelled": lab.numpy(), "w": w.numpy(), "v": v.reshape(-1).numpy()}
    return C, g
