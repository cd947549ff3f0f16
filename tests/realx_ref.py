"""fp64 statement of the objective on real-valued data under the Gaussian decoder with a fixed or a learned per-dimension scale
(include/gmvae_hip.h GMVAE_X_F32, GMVAE_LIK_SCALE_LEARNED), in torch with autograd -- test infrastructure, the checker of
tests/test_realx*.py.  An adapter onto objective_ref.loss_and_grads, as lik_ref is:

    t = x itself (a float array; bytes / 255 for the byte-input case), rows r = b S + s, lambda = the decoder's output
    the networks that read x read t
    log p(t_bd | lambda_rd) = -(lambda_rd - t_bd)^2 / (2 sigma_d^2) - rho_d - ln(2 pi) / 2,   sigma_d = exp(rho_d)
    log w_r = logpx_r + logp_r - logq_r - nent_b,   L_b = -(logsumexp_s log w_bs - ln S)

rho is an extra torch leaf beside objective_ref's own (its gradient is g["decoder/log_sigma"]); with a fixed scalar sigma it is
the constant ln sigma in every dimension and its gradient is reported as 0.  The module also holds the batch and the cases of
the device tests."""
import dataclasses
import math

import numpy as np
import torch

import lik_ref as LR
import objective_ref as OR
import oracle as O

LIK_GAUSSIAN, X_F32, LIK_SCALE_LEARNED = 3 << 11, 1 << 13, 1 << 14      # include/gmvae_hip.h
LOG_SIGMA = "decoder/log_sigma"


def loss_and_grads(model, d: O.Dims, p, x, eps, u=None, sigma=1.0, rho=None, relu_masks=None):
    """model: oracle.MODEL_*; x float [B, D]; eps [B S, L]; u [B S, K] (GMVAE only); rho [D] (the learned scale) or None (the
    fixed scalar sigma).  Returns (C, g) as lik_ref.loss_and_grads does -- C = dict(loss, nll, kl, nent, sqerr, nll_abs, rows,
    bound, lam, mean, pre) -- plus g["decoder/log_sigma"] [D] = d loss / d rho (loss = mean_b L_b), all float64 numpy."""
    B, S = x.shape[0], d.S
    t = np.asarray(x, np.float64)
    tr = torch.tensor(t).repeat_interleave(S, dim=0)
    learned = rho is not None
    rho_t = torch.tensor(np.asarray(rho, np.float64) if learned else np.full(d.D, math.log(float(sigma))), requires_grad=learned)

    def objective(o):
        lam = o["lam"]
        df = lam - tr
        el = -0.5 * df * df * torch.exp(-2.0 * rho_t) - rho_t - 0.5 * OR.LOG_2PI
        logpx = el.sum(dim=1)
        ob = OR.iwae({**o, "logpx": logpx, "lw": logpx + o["logp"] - o["logq"]})
        ob.update(logpx=logpx, lw=logpx + o["logp"] - o["logq"], el=el.detach(), mean=lam.detach())
        return ob

    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    c, g = OR.loss_and_grads(model, d, p, t, eps, objective, S=S, relu_masks=relu_masks, **kw)
    g[LOG_SIGMA] = rho_t.grad.numpy().copy() if learned else np.zeros(d.D)
    C = {"loss": c["loss"], "nll": -c["logpx"].mean().item(), "kl": (c["logq"] - c["logp"]).mean().item(),
         "nent": c["nent"].mean().item(), "bound": -c["Lb"].numpy(), "pre": c["pre"], "lam": c["lam"].numpy(),
         "mean": c["mean"].numpy(), "rows": OR.row_terms({**c, "lw": c["logw"]}),
         "sqerr": ((c["mean"] - tr) ** 2).sum(dim=1).view(B, S).mean(dim=1).sum().item(),
         "nll_abs": c["el"].abs().sum(dim=1).view(B, S).mean(dim=1).mean().item()}
    return C, g


def terms_in(dtype, model, d: O.Dims, p, x, eps, u=None, sigma=1.0, rho=None):
    """The forward of the same statement evaluated in torch `dtype` on the CPU, every operand rounded to it first: dict(rows
    [R, 4] = logpx, logq, logp, log w; loss, nll, kl, nent, sqerr) as float64 numpy.  At torch.float64 it is loss_and_grads'
    forward (tests/test_realx_cpu.py holds the two together); at torch.float32 its distance from that measures what the
    conditioning of a case costs ANY fp32 evaluation, whatever its accumulation order: the device tests allow 4x that
    where it exceeds the standing gate."""
    T = lambda a: torch.tensor(np.asarray(a, np.float64)).to(dtype)
    gm = model == O.MODEL_GMVAE
    B, S, L, K = x.shape[0], d.S, d.L, d.K
    nl = len(d.hidden) + 1
    c, smin = float(d.raw_sigma_bias), float(d.sigma_min)

    def mlp(name, h):
        for i in range(nl):
            h = h @ T(p[f"{name}_fcnet/linear_{i}/w"]) + T(p[f"{name}_fcnet/linear_{i}/b"])
            if i < nl - 1:
                h = OR._act(h, d.act)
        return h

    def mvn(z, mu, sg):
        e = (z - mu) / sg
        return (-0.5 * e * e - 0.5 * OR.LOG_2PI).sum(dim=1) - torch.log(sg).sum(dim=1)

    xt = T(x)
    xr = xt.repeat_interleave(S, dim=0)
    e = T(eps).reshape(B * S, L)
    if gm:
        logits = mlp("encoder_y", xt)
        lnq = torch.log_softmax(logits, dim=1)
        nent = (lnq.exp() * lnq).sum(dim=1)
        pert = logits.repeat_interleave(S, dim=0) - torch.log(-torch.log(T(u).reshape(B * S, K)))
        y = torch.softmax(pert / float(d.temperature), dim=1)
        pp = y @ T(p["prior_gmm_fcnet/linear_0/w"]) + T(p["prior_gmm_fcnet/linear_0/b"])
        qp = mlp("encoder_gmm", torch.cat([xr, y], dim=1))
    else:
        qp = mlp("encoder", xt).repeat_interleave(S, dim=0)
        nent = torch.zeros(B, dtype=dtype)
    mu_q, sig_q = qp[:, :L], torch.clamp(torch.nn.functional.softplus(qp[:, L:] + c), min=smin)
    z = mu_q + sig_q * e
    logq = mvn(z, mu_q, sig_q)
    if gm:
        logp = mvn(z, pp[:, :L], torch.clamp(torch.nn.functional.softplus(pp[:, L:] + c), min=smin))
    elif model == O.MODEL_VAE:
        logp = (-0.5 * z * z - 0.5 * OR.LOG_2PI).sum(dim=1)
    else:
        loc, s = T(p["loc"]), torch.nn.functional.softplus(T(p["raw_scale_diag"]))
        lnw = torch.log_softmax(T(p["mixture_logits"]).reshape(-1), dim=0)
        tt = (z[:, None, :] - loc[None]) / s[None]
        logp = torch.logsumexp(lnw[None] + (-0.5 * tt * tt - 0.5 * OR.LOG_2PI).sum(dim=2) - torch.log(s).sum(dim=1)[None], dim=1)
    lam = mlp("decoder", z) + T(d.gen_bias_init)
    rho_t = T(rho) if rho is not None else T(np.full(d.D, math.log(float(sigma))))
    df = lam - xr
    logpx = (-0.5 * df * df * torch.exp(-2.0 * rho_t) - rho_t - 0.5 * OR.LOG_2PI).sum(dim=1)
    logw = logpx + logp - logq - nent.repeat_interleave(S)
    Lb = -(torch.logsumexp(logw.view(B, S), dim=1) - math.log(S))
    f = lambda v: v.to(torch.float64)
    return {"rows": torch.stack([f(logpx), f(logq), f(logp), f(logw)], dim=1).numpy(), "loss": f(Lb).mean().item(),
            "nll": -f(logpx).mean().item(), "kl": (f(logq) - f(logp)).mean().item(), "nent": f(nent).mean().item(),
            "sqerr": f(df * df).sum(dim=1).view(B, S).mean(dim=1).sum().item()}


def real_batch(B, D, seed=5):
    """(x float32 [B, D], rho float32 [D]): standard normal values, about 10 % exact zeros, a quarter of the columns scaled by
    1e-3 and a quarter by 30; rho uniform per column in [ln 0.05, ln 5]."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, D))
    x[rng.random((B, D)) < 0.1] = 0.0
    scale = np.ones(D)
    cols = rng.permutation(D)
    q = D // 4
    scale[cols[:q]] = 1e-3
    scale[cols[q:2 * q]] = 30.0
    rho = rng.uniform(math.log(0.05), math.log(5.0), size=D)
    return (x * scale).astype(np.float32), rho.astype(np.float32)


# ---- the cases of tests/test_realx.py: every float case runs with the fixed sigma and with the learned rho
@dataclasses.dataclass(frozen=True)
class Case:
    mname: str
    d: object
    B: int
    sigma: float = 0.25          # the fixed-scale variant's sigma
    bytes_in: bool = False       # x as grey-level bytes (t = x / 255): the learned scale alone


CASES = {
    "vae": Case("vae", O.Dims(D=100, L=5, K=1, hidden=(24,)), 9, sigma=0.05),
    "vae_gmp-tanh": Case("vae_gmp", O.Dims(D=100, L=5, K=3, hidden=(24,), sigma_min=0.5, act="tanh"), 9),
    "gmvae-2h": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24), temperature=0.7), 8),
    "gmvae-s3": Case("gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3), 4),                 # row weights into the rho reduction
    "gmvae-d99": Case("gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), 5),                     # unaligned rows: the element path
    "gmvae-784": Case("gmvae", O.Dims(D=784, L=64, K=10, hidden=(64,)), 32),             # interior tiles + the 16-column last tile
    "vae-b1-d3": Case("vae", O.Dims(D=3, L=2, K=1, hidden=(8,)), 1),                         # one row, the reduction's scalar path
    "gmvae-bytes": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24,)), 8, bytes_in=True),
}
SCALES = ("fixed", "learned")
VARIANTS = [(n, s) for n, c in CASES.items() for s in SCALES if not (c.bytes_in and s == "fixed")]


def flags(c: Case, scale):
    return LIK_GAUSSIAN | (0 if c.bytes_in else X_F32) | (LIK_SCALE_LEARNED if scale == "learned" else 0)


def suffix(c: Case, scale):
    return "+gauss" + ("" if c.bytes_in else "+f32") + ("+lsig" if scale == "learned" else "")


def pad4(n):
    return (n + 3) // 4 * 4


def setup(name, scale, seed=0):
    """(model id, Dims, p as the device sees it, flat fp32 -- rho appended as the layout's last entry under the learned scale --,
    x as the device takes it (float32, or uint8 for the byte case), t float64, eps, u, rho float64 or None)."""
    c = CASES[name]
    model = O.MODEL_NAMES[c.mname]
    d = c.d
    rng = np.random.default_rng(seed)
    p = O.init_params(model, d, rng)
    _, eps, u = O.make_inputs(d, c.B, model)
    u = u if model == O.MODEL_GMVAE else None
    xf, rho32 = real_batch(c.B, d.D)
    if c.bytes_in:
        x = LR.grey_batch(c.B, d.D)
        t = LR.targets(x)
    else:
        x, t = xf, xf.astype(np.float64)
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    rho = None
    if scale == "learned":
        tailp = np.zeros(pad4(d.D), np.float32)
        tailp[:d.D] = rho32
        flat = np.concatenate([flat, tailp])
        rho = rho32.astype(np.float64)
    return model, d, p32, flat, x, t, eps, u, rho
