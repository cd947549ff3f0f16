"""fp64 statement of the doubly reparameterised gradient (Tucker et al. 2018; include/gmvae_hip.h GMVAE_GRAD_DREG) for the
importance-weighted objectives, in torch with autograd -- test infrastructure, the checker of tests/test_dreg*.py.

The estimator is stated by stop-gradients, not by its closed form.  With row weights w (the weight the step carries:
softmax_s(log w) for the VAE family, q_bk softmax_s(log w'_bsk) with y summed out, 1 at S = 1) and v = softmax_s(log w) of the
row's own sample group:
    inference parameters (`encoder` / `encoder_gmm`):  the gradient of  sum_b sum_rows (w v).detach() * (-log w_row) / B
        with log q evaluated at mu.detach(), sigma.detach() and z = mu + sigma eps left attached;
    every other parameter:  the gradient of the true loss (mean_b L_b), as tests/ymarg_iw_ref.py / the oracle state it.
estimator="standard" gives the true loss's gradient for every parameter (the plain reparameterised estimator).
The networks, the Gaussian log-density, the ReLU-mask handling and the surrogate pass are tests/objective_ref.py's.
Rows: VAE / VAE_GMP r = b*S + s; GMVAE (y summed out: GMVAE_OBJ_MARGINAL_Y at S = 1, GMVAE_OBJ_MARGINAL_Y_IW) r = (b*S + s)*K + k."""
import objective_ref as OR
import oracle as O
from objective_ref import INFERENCE_NET, is_inference  # noqa: F401


def loss_and_grads(model: int, d: O.Dims, p, x, eps, S: int, relu_masks=None, estimator: str = "dreg"):
    """model: oracle.MODEL_*; d: oracle.Dims (d.S ignored: S is the argument); p: {name: array} (oracle.unpack); x uint8
    [B, D]; eps [rows, L].  The GMVAE is the objective with y summed out (at S = 1: GMVAE_OBJ_MARGINAL_Y).
    Returns (C, g) as tests/ymarg_iw_ref.loss_and_grads: C = dict(loss, nll, kl, nent -- batch means --, per_example [B],
    rows [rows, 4] = logpx, logq, logp, log w, z, pre; GMVAE: logits, dlogits, q; VAE family: dqp [B, 2L] = d (B loss) /
    d (the encoder's output row of example b); dmu, dsig [rows, L] = d (B loss) / d (mu_q, sigma_q) of every row) and
    g = {name: d loss / d param}, all float64 numpy."""
    gm = model == O.MODEL_GMVAE
    kw = dict(objective=OR.summed_out, y="summed") if gm else dict(objective=OR.iwae)
    c, g = OR.loss_and_grads(model, d, p, x, eps, S=S, estimator=estimator, relu_masks=relu_masks, **kw)
    if gm:
        (nll, kl), nent = OR.summed_means(c, c["q"]), c["nent"].mean().item()
    else:
        nll, kl, nent = -c["logpx"].mean().item(), (c["logq"] - c["logp"]).mean().item(), 0.0
    C = {"loss": c["loss"], "nll": nll, "kl": kl, "nent": nent, "per_example": c["Lb"].numpy(), "rows": OR.row_terms(c),
         "z": c["z"].numpy(), "pre": c["pre"], "dmu": c["dmu"], "dsig": c["dsig"], "w": c["w"].numpy(), "v": c["v"].numpy(),
         "sig_q": c["sig_q"].numpy()}
    if gm:
        C.update(logits=c["logits"].numpy(), dlogits=c["dlogits"], q=c["q"].numpy())
    else:
        C["dqp"] = c["dqp"]
    return C, g
