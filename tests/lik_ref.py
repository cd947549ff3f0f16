"""fp64 statement of the objective under a likelihood on grey-level bytes (include/gmvae_hip.h GMVAE_LIK_*), in torch with
autograd -- test infrastructure, the checker of tests/test_lik*.py.

t_bd = x_bd / 255, rows r = b S + s, lambda = the decoder's output:
    the networks that read x (encoder_y, encoder_gmm, encoder) read t
    logpx_r = sum_d [(t_bd lambda_rd - A(lambda_rd)) / phi + c(t_bd)]
    log w_r = logpx_r + logp_r - logq_r - nent_b,   L_b = -(logsumexp_s log w_bs - ln S)      (objective_ref.iwae's, on this logpx)
with (A, A', phi, c) of the likelihood: FAMILY below.  objective_ref.forward runs with x replaced by t (it reads x as a float
array); logpx and log w' are recomputed from its lam.  The continuous Bernoulli's A is a torch.autograd.Function whose backward
is the piecewise A' (a torch.where over the closed form would poison the gradient through its unused 0/0 branch): four series
terms in h = lambda / 2 below |lambda| = 0.05, the expm1 closed forms above -- within 3e-15 of 50-digit arithmetic in both
(tests/test_lik_cpu.py holds them to mpmath).  The module also holds the grey batch and the cases of the device tests."""
import dataclasses
import math

import numpy as np
import torch
import torch.nn.functional as F

import objective_ref as OR
import oracle as O

SERIES_BELOW = 0.05
LIKS = ("grey", "cb", "gauss")
FLAG = {"grey": 1 << 11, "cb": 2 << 11, "gauss": 3 << 11}          # GMVAE_LIK_*
SUFFIX = {"grey": "+grey", "cb": "+cb", "gauss": "+gauss"}          # gmvae_step_schedule's
NAME = {"grey": "grey_bernoulli", "cb": "continuous_bernoulli", "gauss": "gaussian"}      # Engine(likelihood=)


def cb_A(lam):
    """A(lambda) = log((e^lambda - 1) / lambda) of the continuous Bernoulli, A(0) = 0 (float64 tensor in, same shape out)."""
    lam = torch.as_tensor(lam, dtype=torch.float64)
    h = 0.5 * lam
    h2 = h * h
    series = h + h2 / 6.0 - h2 * h2 / 180.0 + h2 * h2 * h2 / 2835.0
    a = lam.abs().clamp(min=SERIES_BELOW)                           # (the closed form's argument where the series is taken: finite)
    closed = lam.clamp(min=0.0) + torch.log(-torch.expm1(-a) / a)
    return torch.where(lam.abs() < SERIES_BELOW, series, closed)


def cb_mean(lam):
    """A'(lambda) = 1 / (1 - e^-lambda) - 1 / lambda, A'(0) = 1/2: the continuous Bernoulli's mean."""
    lam = torch.as_tensor(lam, dtype=torch.float64)
    h = 0.5 * lam
    h2 = h * h
    series = 0.5 + 0.5 * h * (1.0 / 3.0 - h2 / 45.0 + 2.0 * h2 * h2 / 945.0 - h2 * h2 * h2 / 4725.0)
    a = lam.abs().clamp(min=SERIES_BELOW)
    p = 1.0 / (-torch.expm1(-a)) - 1.0 / a                          # A'(|lambda|); A'(-a) = 1 - A'(a)
    closed = torch.where(lam > 0, p, 1.0 - p)
    return torch.where(lam.abs() < SERIES_BELOW, series, closed)


class _CbA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lam):
        ctx.save_for_backward(lam)
        return cb_A(lam)

    @staticmethod
    def backward(ctx, g):
        (lam,) = ctx.saved_tensors
        return g * cb_mean(lam)


def family(lik, sigma=1.0):
    """(A, A', phi, c) of the likelihood: callables on float64 tensors, phi a float."""
    if lik == "grey":
        return F.softplus, torch.sigmoid, 1.0, lambda t: torch.zeros_like(t)
    if lik == "cb":
        return _CbA.apply, cb_mean, 1.0, lambda t: torch.zeros_like(t)
    if lik == "gauss":
        s = float(sigma)
        return (lambda l: 0.5 * l * l), (lambda l: l), s * s, lambda t: -t * t / (2.0 * s * s) - math.log(s) - 0.5 * OR.LOG_2PI
    raise ValueError(lik)


def targets(x):
    """t = x / 255 (float64 numpy) of a uint8 grey batch."""
    return np.asarray(x, np.float64) / 255.0


def loss_and_grads(model, d: O.Dims, p, x, eps, u=None, lik="cb", sigma=1.0, relu_masks=None):
    """model: oracle.MODEL_*; x uint8 grey levels [B, D]; eps [B S, L]; u [B S, K] (GMVAE only).  Returns (C, g): C = dict(loss,
    nll, kl, nent -- batch means, nll / kl averaged over s --, sqerr = sum_b mean_s sum_d (A' - t)^2, nll_abs = mean_b mean_s
    sum_d |(t lambda - A) / phi + c|, rows [R, 4] = logpx, logq, logp, log w, bound [B], lam, mean = A'(lambda), pre = per-net
    pre-activations) and g = {name: d loss / d param} (loss = mean_b L_b), all float64 numpy."""
    B, S = x.shape[0], d.S
    t = targets(x)
    A, Ap, phi, cfn = family(lik, sigma)
    tr = torch.tensor(t).repeat_interleave(S, dim=0)

    def objective(o):
        lam = o["lam"]
        el = (tr * lam - A(lam)) / phi + cfn(tr)
        logpx = el.sum(dim=1)
        ob = OR.iwae({**o, "logpx": logpx, "lw": logpx + o["logp"] - o["logq"]})
        ob.update(logpx=logpx, lw=logpx + o["logp"] - o["logq"], el=el.detach(), mean=Ap(lam.detach()))
        return ob

    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    c, g = OR.loss_and_grads(model, d, p, t, eps, objective, S=S, relu_masks=relu_masks, **kw)
    C = {"loss": c["loss"], "nll": -c["logpx"].mean().item(), "kl": (c["logq"] - c["logp"]).mean().item(),
         "nent": c["nent"].mean().item(), "bound": -c["Lb"].numpy(), "pre": c["pre"], "lam": c["lam"].numpy(),
         "mean": c["mean"].numpy(), "rows": OR.row_terms({**c, "lw": c["logw"]}),
         "sqerr": ((c["mean"] - tr) ** 2).sum(dim=1).view(B, S).mean(dim=1).sum().item(),
         "nll_abs": c["el"].abs().sum(dim=1).view(B, S).mean(dim=1).mean().item()}
    return C, g


# ---- the grey batch of every case
def grey_batch(B, D, seed=5):
    """uint8 [B, D]: integers 0..255, then about 30 % forced to 0 and 10 % to 255."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(B, D))
    r = rng.random((B, D))
    x[r < 0.3] = 0
    x[r >= 0.9] = 255
    return x.astype(np.uint8)


# ---- the cases of tests/test_lik.py
@dataclasses.dataclass(frozen=True)
class Case:
    mname: str
    d: object
    B: int
    lik: str
    sigma: float = 1.0
    bias_vec: bool = False       # gen_bias_init as a [D] vector (GmvaeDims::gen_bias_vec)
    lam_scale: float = None      # the decoder's last layer scaled so that max |lambda| is about this; 0.0: weight and bias exactly 0


_VAE = O.Dims(D=100, L=5, K=1, hidden=(24,))
_G784 = O.Dims(D=784, L=64, K=10, hidden=(64,))
# gumbel-784-*: the logits launch of 784 columns takes the small tile configuration (32 x 32), whose interior path needs a whole
# 32-row tile: B = 16 would send every tile down the element path, so these cases run B = 32 -- 24 interior column tiles and the
# 16-column last tile
B784 = 32
CASES = {
    "vae-grey": Case("vae", _VAE, 9, "grey"),
    "vae_gmp-cb": Case("vae_gmp", O.Dims(D=100, L=5, K=3, hidden=(24,), sigma_min=0.5), 9, "cb"),
    "gumbel-cb": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24), temperature=0.7), 8, "cb"),
    "gmvae-s3-gauss": Case("gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3), 4, "gauss", sigma=0.25),
    "vae-s3-cb": Case("vae", O.Dims(D=96, L=4, K=1, hidden=(16,), S=3), 4, "cb"),
    "gumbel-d99-cb": Case("gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), 5, "cb"),                  # unaligned rows: the element path
    "gumbel-d99-gauss": Case("gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), 5, "gauss", sigma=1.0),
    "gumbel-784-grey": Case("gmvae", _G784, B784, "grey"),
    "gumbel-784-cb": Case("gmvae", _G784, B784, "cb"),
    "gumbel-784-gauss": Case("gmvae", _G784, B784, "gauss", sigma=0.25),
    "vae_gmp-tanh-gauss": Case("vae_gmp", O.Dims(D=100, L=5, K=3, hidden=(24,), sigma_min=0.5, act="tanh"), 9, "gauss", sigma=1.0),
    "gumbel-bias-vec-cb": Case("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24,)), 8, "cb", bias_vec=True),
    "vae-cb-tiny": Case("vae", _VAE, 9, "cb", lam_scale=0.9e-3),
    "vae-cb-saturated": Case("vae", _VAE, 9, "cb", lam_scale=60.0),
    "vae-cb-100": Case("vae", _VAE, 9, "cb", lam_scale=100.0),
    "vae-cb-zero": Case("vae", _VAE, 9, "cb", lam_scale=0.0),
    "vae-gauss-sigma-small": Case("vae", _VAE, 9, "gauss", sigma=0.05),
}
# the cases of the train-graph tests that are no row of the table above: (model name, Dims, likelihood, sigma)
GRAPH_CASES = {"gumbel-cb": ("gmvae", CASES["gumbel-cb"].d, "cb", 1.0),
               "vae-s3-gauss": ("vae", CASES["vae-s3-cb"].d, "gauss", 0.25)}


def setup(name, seed=0):
    """(model id, Dims, p as the device sees it, flat fp32, x uint8 grey levels, eps, u)."""
    c = CASES[name]
    model = O.MODEL_NAMES[c.mname]
    d = c.d
    rng = np.random.default_rng(seed)
    if c.bias_vec:
        d = dataclasses.replace(d, gen_bias_init=np.linspace(-1.5, 1.5, d.D).astype(np.float32))
    p = O.init_params(model, d, rng)
    _, eps, u = O.make_inputs(d, c.B, model)
    x = grey_batch(c.B, d.D)
    u = u if model == O.MODEL_GMVAE else None
    if c.lam_scale is not None:
        nl = len(d.hidden)
        wn, bn = f"decoder_fcnet/linear_{nl}/w", f"decoder_fcnet/linear_{nl}/b"
        p = dict(p)
        if c.lam_scale == 0.0:
            p[wn], p[bn] = np.zeros_like(p[wn]), np.zeros_like(p[bn])
        else:
            f = c.lam_scale / np.abs(decoder_logits(model, d, p, x, eps, u)).max()
            p[wn], p[bn] = p[wn] * f, p[bn] * f
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    return model, d, p32, flat, x, eps, u


def decoder_logits(model, d, p, x, eps, u):
    """The decoder's logits of the forward on t = x / 255."""
    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    return OR.forward(model, d, OR.leaves(p), targets(x), eps, S=d.S, **kw)["lam"].detach().numpy()
