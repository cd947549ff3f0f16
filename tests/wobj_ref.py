"""fp64 statement of the weighted objective (include/gmvae_hip.h GMVAE_OBJ_WEIGHTS, S = 1), in torch with autograd through the
max -- test infrastructure, the checker of tests/test_wobj*.py.

With nll = -log p(x|z), kl = log q(z|.) - log p(z|.) and nent_b = sum_k q_bk ln q_bk (KL(q(y|x_b) || uniform) = nent_b + ln K; the
ln K stays out of the loss, as in the reference):
    vae, vae_gmp:          L_b = nll_b + beta_z kl_b                                   (beta_y, lambda ignored)
    gmvae, Gumbel y:       L_b = nll_b + beta_z kl_b + beta_y ne'_b                    (u: the Gumbel draw, scripts/gmvae.py:238-240)
    gmvae, y summed out:   L_b = sum_k q_bk (nll_bk + beta_z kl_bk) + beta_y ne'_b     (rows r = b K + k, tests/ymarg_ref.py)
    ne'_b = max(nent_b, lambda - ln K);  lambda == 0: ne'_b = nent_b (no floor, whatever the rounding)
Parameters as oracle.unpack gives them; per-net ReLU masks as oracle.loss_and_grads takes them."""
import math

import numpy as np

import objective_ref as OR
import oracle as O


def loss_and_grads(model, d: O.Dims, p, x, eps, u=None, weights=(1.0, 1.0, 0.0), marginal=False, relu_masks=None):
    """model: oracle.MODEL_*; x uint8 [B, D]; eps [R, L], R = B (B K with marginal); u [B, K] (Gumbel GMVAE only);
    weights = (beta_z, beta_y, lambda).  Returns (C, g): C = dict(loss, nll, kl, nent -- batch means; nll, kl, nent unweighted --,
    kl_y [B] = nent_b + ln K, floor [B] = 1 - a_b, q [B, K] = softmax(logits) (GMVAE), pre = per-net pre-activations) and g = {name: d loss / d param}
    (loss = mean_b L_b), all float64 numpy."""
    gm = model == O.MODEL_GMVAE
    assert gm or not marginal
    kw = dict(y="summed" if marginal else "gumbel", u=u) if gm else {}
    c, g = OR.loss_and_grads(model, d, p, x, eps, lambda o: OR.weighted(o, weights, marginal), relu_masks=relu_masks, **kw)
    C = {"loss": c["loss"], "nll": c["nll_b"].mean().item(), "kl": c["kl_b"].mean().item(), "nent": c["nent"].mean().item(),
         "kl_y": c["nent"].numpy() + (math.log(d.K) if gm else 0.0), "floor": c["floor"], "pre": c["pre"],
         "q": c["q"].numpy() if gm else None}
    return C, g


def split_lambda(kl_y, min_gap=1e-3):
    """The lambda of the GPU tests: the midpoint of the widest gap between two neighbouring sorted values of KL_y over the batch,
    so that the floor holds for some examples and not for others.  Asserts the issue's condition: the two values differ by more
    than min_gap nats (both groups are non-empty by construction)."""
    v = np.sort(np.asarray(kl_y, np.float64))
    i = int(np.argmax(np.diff(v)))
    assert v[i + 1] - v[i] > min_gap, f"KL_y values too close for a stable split: gap {v[i + 1] - v[i]:.3e}"
    lam = 0.5 * (v[i] + v[i + 1])
    assert (kl_y < lam).any() and (kl_y > lam).any()
    return lam


# ---- the shapes of tests/test_wobj.py (model, marginal, Dims, B); tests/test_wobj_cpu.py checks their lambda condition in fp64
CASES = {
    "vae": ("vae", False, O.Dims(D=100, L=5, K=1, hidden=(24,)), 9),
    "vae_gmp": ("vae_gmp", False, O.Dims(D=100, L=5, K=3, hidden=(24,), sigma_min=0.5), 9),
    "gumbel": ("gmvae", False, O.Dims(D=100, L=5, K=7, hidden=(24, 24), temperature=0.7), 8),
    "marginal": ("gmvae", True, O.Dims(D=100, L=5, K=7, hidden=(24, 24)), 8),
    "marginal-K80": ("gmvae", True, O.Dims(D=64, L=4, K=80, hidden=(16,)), 5),
    "gumbel-K80": ("gmvae", False, O.Dims(D=64, L=4, K=80, hidden=(16,)), 5),
    "gumbel-one-launch-sizes": ("gmvae", False, O.Dims(D=784, L=64, K=10, hidden=(64,)), 16),
    "marginal-one-launch-sizes": ("gmvae", True, O.Dims(D=784, L=64, K=10, hidden=(64,)), 16),
}
WEIGHTS = (0.25, 2.0)          # (beta_z, beta_y) of the parity cases; lambda: split_lambda of the case's own KL_y


def setup(name, seed=0):
    """(model id, marginal, Dims, p as the device sees it, flat fp32, x, eps, u) of a case: Xavier parameters from `seed`, the
    oracle's synthetic inputs."""
    mname, marginal, d, B = CASES[name]
    model = O.MODEL_NAMES[mname]
    p = O.init_params(model, d, np.random.default_rng(seed))
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    dn = O.Dims(**{**d.__dict__, "S": d.K}) if marginal else d
    x, eps, u = O.make_inputs(dn, B, model)
    return model, marginal, d, p32, flat, x, eps, (None if marginal else u)


def case_lambda(name):
    """lambda of a case: split on the fp64 statement's own KL_y (0 for the VAE family, which has no y term)."""
    model, marginal, d, p32, flat, x, eps, u = setup(name)
    if model != O.MODEL_GMVAE:
        return 0.0
    C, _ = loss_and_grads(model, d, p32, x, eps, u, (1.0, 1.0, 0.0), marginal)
    return split_lambda(C["kl_y"])
