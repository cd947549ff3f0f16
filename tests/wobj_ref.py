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
import torch
import torch.nn.functional as F

import oracle as O
from ymarg_ref import LOG_2PI, _mlp, _mvn_logprob


def loss_and_grads(model, d: O.Dims, p, x, eps, u=None, weights=(1.0, 1.0, 0.0), marginal=False, relu_masks=None):
    """model: oracle.MODEL_*; x uint8 [B, D]; eps [R, L], R = B (B K with marginal); u [B, K] (Gumbel GMVAE only);
    weights = (beta_z, beta_y, lambda).  Returns (C, g): C = dict(loss, nll, kl, nent -- batch means; nll, kl, nent unweighted --,
    kl_y [B] = nent_b + ln K, floor [B] = 1 - a_b, q [B, K] = softmax(logits) (GMVAE), pre = per-net pre-activations) and g = {name: d loss / d param}
    (loss = mean_b L_b), all float64 numpy."""
    rm = relu_masks or {}
    bz, by, lam = (float(w) for w in weights)
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    B, K, L = x.shape[0], d.K, d.L
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)
    xf = torch.tensor(np.asarray(x), dtype=torch.float64)
    gm = model == O.MODEL_GMVAE
    assert gm or not marginal
    rpx = K if marginal else 1
    R = B * rpx
    eps = torch.tensor(np.asarray(eps, np.float64).reshape(R, L))
    pre = {}
    q = None
    nent = torch.zeros(B, dtype=torch.float64)
    if gm:
        pre = {"encoder_y": [], "encoder_gmm": [], "decoder": []}
        logits = _mlp(t, "encoder_y", nl, xf, d.act, rm.get("encoder_y"), pre["encoder_y"])
        lnq = torch.log_softmax(logits, dim=1)
        q = lnq.exp()
        nent = (q * lnq).sum(dim=1)
        if marginal:
            y = torch.eye(K, dtype=torch.float64).repeat(B, 1)
        else:
            ut = torch.tensor(np.asarray(u, np.float64).reshape(B, K))
            y = torch.softmax((logits - torch.log(-torch.log(ut))) / float(d.temperature), dim=1)
        xr = xf.repeat_interleave(rpx, dim=0)
        pp = y @ t["prior_gmm_fcnet/linear_0/w"] + t["prior_gmm_fcnet/linear_0/b"]
        qp = _mlp(t, "encoder_gmm", nl, torch.cat([xr, y], dim=1), d.act, rm.get("encoder_gmm"), pre["encoder_gmm"])
    else:
        pre = {"encoder": [], "decoder": []}
        xr = xf
        qp = _mlp(t, "encoder", nl, xf, d.act, rm.get("encoder"), pre["encoder"])
    mu_q, sig_q = qp[:, :L], torch.clamp(F.softplus(qp[:, L:] + c), min=smin)
    z = mu_q + sig_q * eps
    logq = _mvn_logprob(z, mu_q, sig_q)
    if gm:
        mu_p, sig_p = pp[:, :L], torch.clamp(F.softplus(pp[:, L:] + c), min=smin)
        logp = _mvn_logprob(z, mu_p, sig_p)
    elif model == O.MODEL_VAE:
        logp = (-0.5 * z * z - 0.5 * LOG_2PI).sum(dim=1)
    else:
        loc, s = t["loc"], F.softplus(t["raw_scale_diag"])
        lnw = torch.log_softmax(t["mixture_logits"], dim=0)
        tt = (z[:, None, :] - loc[None]) / s[None]
        lnN = (-0.5 * tt * tt - 0.5 * LOG_2PI).sum(dim=2) - torch.log(s).sum(dim=1)[None]
        logp = torch.logsumexp(lnw[None] + lnN, dim=1)
    lam_d = _mlp(t, "decoder", nl, z, d.act, rm.get("decoder"), pre["decoder"])
    lam_d = lam_d + torch.as_tensor(np.asarray(d.gen_bias_init, np.float64))
    logpx = (xr * lam_d - F.softplus(lam_d)).sum(dim=1)
    nll_r, kl_r = -logpx, logq - logp
    if marginal:
        nll_b, kl_b = (q * nll_r.view(B, K)).sum(dim=1), (q * kl_r.view(B, K)).sum(dim=1)
    else:
        nll_b, kl_b = nll_r, kl_r
    Lb = nll_b + bz * kl_b
    floor = np.zeros(B)
    if gm:
        thr = lam - math.log(K)
        if lam == 0.0:
            nef = nent
        else:
            nef = torch.clamp(nent, min=thr)                       # (autograd through the max: no gradient below the floor)
            floor = (nent.detach().numpy() <= thr).astype(np.float64)
        Lb = Lb + by * nef
    loss = Lb.mean()
    loss.backward()
    g = {k: v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy()) for k, v in t.items()}
    C = {"loss": loss.item(), "nll": nll_b.mean().item(), "kl": kl_b.mean().item(), "nent": nent.mean().item(),
         "kl_y": nent.detach().numpy() + (math.log(K) if gm else 0.0), "floor": floor, "pre": pre,
         "q": q.detach().numpy() if gm else None}
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
