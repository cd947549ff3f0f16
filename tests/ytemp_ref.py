"""fp64 statement of the Gumbel GMVAE's step with the temperature as an argument and the straight-through y (include/gmvae_hip.h
GMVAE_Y_TEMP_DEV, GMVAE_Y_STRAIGHT_THROUGH), in torch with autograd -- test infrastructure, the checker of tests/test_ytemp*.py.

With g = -ln(-ln u), a_rk = (logits_bk + g_rk) / tau and y_soft = softmax_k a_rk (row r = b S + s):
    relaxed:            y = y_soft                                            (scripts/gmvae.py:238-240)
    straight-through:   y = y_soft + (y_hard - y_soft).detach(),  y_hard = e_{argmax_k (logits_bk + g_rk)} (lowest index on ties)
    log w_r = log p(x_b|z_r) + log p(z_r|y_r) - log q(z_r|x_b,y_r) - nent_b,  nent_b = sum_k q_bk ln q_bk
    L_b = -(logsumexp_s log w_bs - ln S);   at S = 1 with weights (beta_z, beta_y, 0): L_b = nll_b + beta_z kl_b + beta_y nent_b
Parameters as oracle.unpack gives them; per-net ReLU masks as oracle.loss_and_grads takes them."""
import numpy as np
import torch

import objective_ref as OR
import oracle as O


def loss_and_grads(d: O.Dims, p, x, eps, u, tau, straight_through=False, weights=None, relu_masks=None, y_leaf=False):
    """x uint8 [B, D]; eps [B S, L]; u [B S, K]; tau: the temperature (d.temperature is NOT read); weights: None or (beta_z,
    beta_y, 0) at S = 1.  y_leaf: y is the LEAF y_hard (no path back to the logits): C["dy"] = d loss / d y there, and the
    logits' gradient keeps the entropy term alone.
    Returns (C, g): C = dict(loss, nll, kl, nent -- batch means, nll and kl means over s too --, logits [B, K], dlogits [B, K] =
    d loss / d logits, y [R, K] as consumed, y_soft [R, K], argmax [R], gap [R] = the top-two gap of logits + g per row, pre =
    per-net pre-activations) and g = {name: d loss / d param} (loss = mean_b L_b), all float64 numpy."""
    objective = OR.iwae
    if weights is not None:
        assert d.S == 1 and float(weights[2]) == 0.0
        objective = lambda o: OR.weighted(o, weights)
    c, g = OR.loss_and_grads(O.MODEL_GMVAE, d, p, x, eps, objective, S=d.S, y="leaf" if y_leaf else "gumbel", u=u, tau=tau,
                             straight_through=straight_through, relu_masks=relu_masks)
    top2 = torch.topk(c["pert"], 2, dim=1).values
    C = {"loss": c["loss"], "nll": -c["logpx"].mean().item(), "kl": (c["logq"] - c["logp"]).mean().item(),
         "nent": c["nent"].mean().item(), "logits": c["logits"].numpy(), "dlogits": c["dlogits"], "y": c["y"].numpy(),
         "y_soft": c["y_soft"].numpy(), "argmax": c["pert"].argmax(dim=1).numpy(), "gap": (top2[:, 0] - top2[:, 1]).numpy(),
         "pre": c["pre"], "dy": c["dy"]}
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
