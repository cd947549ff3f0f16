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


def real_batch(B, D, seed=5, big=30.0, sigma_lo=0.05):
    """(x float32 [B, D], rho float32 [D]): standard normal values, about 10 % exact zeros, a quarter of the columns scaled by
    1e-3 and a quarter by `big` = 30; rho uniform per column in [ln sigma_lo, ln 5], sigma_lo = 0.05."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, D))
    x[rng.random((B, D)) < 0.1] = 0.0
    scale = np.ones(D)
    cols = rng.permutation(D)
    q = D // 4
    scale[cols[:q]] = 1e-3
    scale[cols[q:2 * q]] = big
    rho = rng.uniform(math.log(sigma_lo), math.log(5.0), size=D)
    return (x * scale).astype(np.float32), rho.astype(np.float32)


# ---- the cases of tests/test_realx.py: every float case runs with the fixed sigma and with the learned rho
@dataclasses.dataclass(frozen=True)
class Case:
    mname: str
    d: object
    B: int
    sigma: float = 0.25          # the fixed-scale variant's sigma
    bytes_in: bool = False       # x as grey-level bytes (t = x / 255): the learned scale alone
    big: float = 30.0            # real_batch's scale of its large columns
    sigma_lo: float = 0.05       # ... and the lower end of its sigma range


CASES = {
    "vae": Case("vae", O.Dims(D=100, L=5, K=1, hidden=(24,)), 9, sigma=0.05),
    "vae_gmp-tanh": Case("vae_gmp", O.Dims(D=100, L=5, K=3, hidden=(24,), sigma_min=0.5, act="tanh"), 9),
    "gmvae-2h": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24), temperature=0.7), 8),
    "gmvae-s3": Case("gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3), 4),                 # row weights into the rho reduction
    "gmvae-d99": Case("gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), 5),                     # unaligned rows: the element path
    "gmvae-784": Case("gmvae", O.Dims(D=784, L=64, K=10, hidden=(64,)), 32),             # interior tiles + the 16-column last tile
    "vae-b1-d3": Case("vae", O.Dims(D=3, L=2, K=1, hidden=(8,)), 1),                         # one row, the reduction's scalar path
    "gmvae-bytes": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24,)), 8, bytes_in=True),
    # rho's reduction (csrc/liksig.hpp) beyond one row slab -- R = B S rows in slabs of rs = 64 rows, doubled until at most 256
    # slabs; strips of 64 columns -- and the weight gradients under NS = num_splits(R) > 1 split-K slabs:
    # 3 slabs, the last with 2 rows; two column strips, the second with 36 columns; no row weights
    "vae-r130": Case("vae", O.Dims(D=100, L=5, K=1, hidden=(24,)), 130),
    # 11 slabs on the scalar path (D % 4 != 0), the row weights live; NS = 2 with NSB = num_splits(B) = 1: liksig_finish zeroes
    # slab 1, and the float x's weight gradients lie on fewer slabs than the rest
    "gmvae-r650": Case("gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,), S=5), 130),
    # rs doubles to 128: 129 slabs, the last with 66 rows, eight rows per thread; NS = 16; a 4-column last strip on the vector path
    # Its batch is milder (large columns x 3, sigma >= 0.5): under S = 50 the row weights are softmax_s(log w), an ABSOLUTE error
    # of log w is a relative error of every gradient, and with the x 30 columns under sigma = 0.05 |log p(x|z)| is 4e5 per row,
    # where one fp32 rounding is 0.03 -- the fp64 statement with log p(x|z) merely rounded to fp32 then sits 4e-5 of max |g| off,
    # the whole statement in torch fp32 on the CPU 7e-3 (the device: 2.8e-4).  With this batch: 1e-6 and 6e-6.
    "vae-r16450": Case("vae", O.Dims(D=68, L=4, K=1, hidden=(16,), S=50), 329, sigma=0.5, big=3.0, sigma_lo=0.5),
}
BEYOND_ONE_SLAB = ("vae-r130", "gmvae-r650", "vae-r16450")
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
    xf, rho32 = real_batch(c.B, d.D, big=c.big, sigma_lo=c.sigma_lo)
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


# ---- rho's reduction as csrc/liksig.hpp orders it, in fp32
LSIG_ROW_LANES, LSIG_MAX_SLABS = 16, 256      # liksig.hpp kLsigRowLanes, kLsigMaxSlabs


def liksig_slab_rows(R):
    """liksig.hpp liksig_slab_rows: 64 rows per slab, doubled until at most 256 slabs."""
    rs = 64
    while (R + rs - 1) // rs > LSIG_MAX_SLABS:
        rs *= 2
    return rs


def rho_terms(C, t, rho, S):
    """What the reduction reads, from the statement: g = (lambda - t) / sigma^2 [R, D] and the row weights [R] -- softmax_s of
    log w within an example (all 1 at S = 1) -- as float64."""
    R = C["lam"].shape[0]
    g = (C["lam"] - np.repeat(np.asarray(t, np.float64), S, axis=0)) * np.exp(-2.0 * rho)[None, :]
    lw = C["rows"][:, 3].reshape(R // S, S)
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    return g, (w / w.sum(axis=1, keepdims=True)).reshape(R)


def rho_reduction(g, rw, rho, dtype=np.float32):
    """sum_r rw_r (1 - sigma_d^2 g_rd^2) [D] in `dtype`, in liksig_partial / liksig_finish's order: each of the 16 row lanes of a
    slab sums its rows (every 16th) in index order with the kernel's two fused multiply-adds per element, the 16 lanes are summed
    in lane order, then the slabs in index order.  (A fused multiply-add of float32 operands is formed in float64 -- the product
    is exact there -- and rounded once more to float32.)"""
    f = dtype
    R, D = g.shape
    rs = liksig_slab_rows(R)
    ns = (R + rs - 1) // rs
    G, W = np.zeros((ns * rs, D), f), np.zeros(ns * rs, f)      # (rows beyond R: weight 0, fma(0, ., acc) == acc)
    G[:R], W[:R] = g, rw
    G, W = G.reshape(ns, rs // LSIG_ROW_LANES, LSIG_ROW_LANES, D), W.reshape(ns, rs // LSIG_ROW_LANES, LSIG_ROW_LANES)
    s2 = np.exp(f(2.0) * np.asarray(rho, f)).astype(f)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c).astype(f)
    acc = np.zeros((ns, LSIG_ROW_LANES, D), f)
    for i in range(rs // LSIG_ROW_LANES):
        c = G[:, i]
        inner = fma((-s2[None, None, :] * c).astype(f), c, 1.0)
        acc = fma(np.broadcast_to(W[:, i][:, :, None], inner.shape), inner, acc.astype(np.float64))
    part = np.zeros((ns, D), f)
    for k in range(LSIG_ROW_LANES):
        part = (part + acc[:, k]).astype(f)
    tot = np.zeros(D, f)
    for s in range(ns):
        tot = (tot + part[s]).astype(f)
    return tot.astype(np.float64)
