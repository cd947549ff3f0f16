"""fp64 statement of the objective on count data under the Poisson and the negative-binomial decoder (include/gmvae_hip.h
GMVAE_LIK_POISSON, GMVAE_LIK_NEG_BINOMIAL) -- test infrastructure, the checker of tests/test_count*.py.

    x float [B, D] >= 0; rows r = b S + s; lambda = the decoder's output, the LOG-mean; the networks that read x read log1p(x)
    poisson   log p = x l - exp(l) - lgamma(x + 1)                                        g = exp(l) - x
    nb        r_d = exp(rho_d), u = l - rho_d, sp = softplus
              log p = lgamma(x + r) - lgamma(r) - lgamma(x + 1) - x sp(-u) - r sp(u)      g = (r + x) sigmoid(u) - x
              d log p / d rho = r [psi(x + r) - psi(r) - sp(u)] + g
    tail[5] = sum_b mean_s sum_d (log1p(exp lambda_rd) - log1p(x_bd))^2,  tail[6] = B D,  tail[7] = 0

The element-wise part is stated in NumPy (log_prob, grad_logit, grad_rho, with a digamma and an lgamma difference of its own) and
anchored by torch.distributions with fp64 autograd in tests/test_count_cpu.py; the whole step is an adapter onto
objective_ref.loss_and_grads, as lik_ref and realx_ref are, with rho an extra torch leaf (g["decoder/log_dispersion"]); one TF-Adam
step is adam_ref's statement on the gradient sums.  The module also holds the batches and the cases of the device tests."""
import dataclasses
import math

import numpy as np
import torch

import objective_ref as OR
import oracle as O

X_F32, LIK_POISSON, LIK_NEG_BINOMIAL = 1 << 13, 1 << 15, 1 << 16      # include/gmvae_hip.h
LOG_DISPERSION = "decoder/log_dispersion"
KINDS = ("poisson", "nb")
FLAG = {"poisson": LIK_POISSON | X_F32, "nb": LIK_NEG_BINOMIAL | X_F32}
SUFFIX = {"poisson": "+pois+f32", "nb": "+nb+f32"}
NAME = {"poisson": "poisson", "nb": "negative_binomial"}
EULER_GAMMA = 0.57721566490153286


# ---- the element-wise statement in NumPy
def softplus(v):
    v = np.asarray(v, np.float64)
    return np.maximum(v, 0.0) + np.log1p(np.exp(-np.abs(v)))


def sigmoid(v):
    v = np.asarray(v, np.float64)
    a = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + a), a / (1.0 + a))


def digamma(v):
    """psi(v), v > 0: the recurrence psi(v) = psi(v + 1) - 1 / v up to an argument >= 6, then the asymptotic series to 1 / v^12."""
    v = np.array(v, np.float64, copy=True)
    s = np.zeros_like(v)
    while True:
        lo = v < 6.0
        if not lo.any():
            break
        s = np.where(lo, s - 1.0 / np.where(lo, v, 1.0), s)
        v = np.where(lo, v + 1.0, v)
    i = 1.0 / v
    i2 = i * i
    ser = i2 * (1 / 12 - i2 * (1 / 120 - i2 * (1 / 252 - i2 * (1 / 240 - i2 * (1 / 132 - i2 * (691 / 32760))))))
    return s + np.log(v) - 0.5 * i - ser


_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def lgamma_diff(x, r):
    """lgamma(x + r) - lgamma(r) in fp64; exactly 0 at x = 0."""
    x, r = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(r, np.float64))
    return np.where(x > 0, _lgamma(x + r) - _lgamma(r), 0.0)


def log_prob(kind, x, lam, rho=None):
    """log p(x | lambda) per element, float64."""
    x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
    if kind == "poisson":
        return x * lam - np.exp(lam) - _lgamma(x + 1.0)
    r, u = np.exp(rho), lam - rho
    return lgamma_diff(x, r) - _lgamma(x + 1.0) - x * softplus(-u) - r * softplus(u)


def grad_logit(kind, x, lam, rho=None):
    """g = d (-log p) / d lambda per element."""
    x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
    if kind == "poisson":
        return np.exp(lam) - x
    r, u = np.exp(rho), lam - rho
    return r * sigmoid(u) - x * sigmoid(-u)


def grad_rho(x, lam, rho):
    """d log p / d rho per element (the negative binomial)."""
    x, lam = np.asarray(x, np.float64), np.asarray(lam, np.float64)
    r, u = np.exp(rho), lam - rho
    dps = np.where(x > 0, digamma(x + r) - digamma(r * np.ones_like(x)), 0.0)
    return r * (dps - softplus(u)) + grad_logit("nb", x, lam, rho)


def sq_term(x, lam):
    """(log1p(exp lambda) - log1p(x))^2 per element: tail[5]'s addend."""
    return (softplus(lam) - np.log1p(np.asarray(x, np.float64))) ** 2


# ---- the whole step: an adapter onto objective_ref
def _t_softplus(v):
    return torch.clamp(v, min=0.0) + torch.log1p(torch.exp(-v.abs()))


def loss_and_grads(model, d: O.Dims, p, x, eps, u=None, kind="poisson", rho=None, relu_masks=None):
    """model: oracle.MODEL_*; x float [B, D] counts; eps [B S, L]; u [B S, K] (GMVAE only); rho [D] (kind "nb").  Returns (C, g):
    C = dict(loss, nll, kl, nent, sqerr, nll_abs, rows, bound, lam, pre), g = {name: d loss / d param} with
    g["decoder/log_dispersion"] [D] (zeros under the Poisson), loss = mean_b L_b, all float64 numpy."""
    B, S = x.shape[0], d.S
    xx = np.asarray(x, np.float64)
    xr = torch.tensor(xx).repeat_interleave(S, dim=0)
    nb = kind == "nb"
    rho_t = torch.tensor(np.asarray(rho, np.float64) if nb else np.zeros(d.D), requires_grad=nb)

    def objective(o):
        lam = o["lam"]
        if nb:
            r, uu = torch.exp(rho_t), lam - rho_t
            el = torch.lgamma(xr + r) - torch.lgamma(r) - torch.lgamma(xr + 1.0) - xr * _t_softplus(-uu) - r * _t_softplus(uu)
        else:
            el = xr * lam - torch.exp(lam) - torch.lgamma(xr + 1.0)
        logpx = el.sum(dim=1)
        ob = OR.iwae({**o, "logpx": logpx, "lw": logpx + o["logp"] - o["logq"]})
        ob.update(logpx=logpx, lw=logpx + o["logp"] - o["logq"], el=el.detach())
        return ob

    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    c, g = OR.loss_and_grads(model, d, p, np.log1p(xx), eps, objective, S=S, relu_masks=relu_masks, **kw)
    g[LOG_DISPERSION] = rho_t.grad.numpy().copy() if nb else np.zeros(d.D)
    lam = c["lam"].numpy()
    C = {"loss": c["loss"], "nll": -c["logpx"].mean().item(), "kl": (c["logq"] - c["logp"]).mean().item(),
         "nent": c["nent"].mean().item(), "bound": -c["Lb"].numpy(), "pre": c["pre"], "lam": lam,
         "rows": OR.row_terms({**c, "lw": c["logw"]}),
         "sqerr": sq_term(np.repeat(xx, S, axis=0), lam).sum(axis=1).reshape(B, S).mean(axis=1).sum(),
         "nll_abs": c["el"].abs().sum(dim=1).view(B, S).mean(dim=1).mean().item()}
    return C, g


def row_weights(C, S):
    """The backward's row weights [R]: softmax_s of log w within an example (all 1 at S = 1)."""
    R = C["lam"].shape[0]
    lw = C["rows"][:, 3].reshape(R // S, S)
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    return (w / w.sum(axis=1, keepdims=True)).reshape(R)


# ---- batches
def count_batch(B, D, seed=5, top=200.0):
    """(x float32 [B, D] counts, rho float32 [D]): gamma-Poisson draws with per-column means spread over exp(N(0, 1.5)), about
    a third of the entries exactly 0, the largest scaled up to `top`; rho uniform per column in [-2, 3]."""
    rng = np.random.default_rng(seed)
    mean = np.exp(rng.normal(0.0, 1.5, (1, D))) * np.exp(rng.normal(0.0, 0.5, (B, D)))
    x = rng.poisson(rng.gamma(1.0, mean)).astype(np.float64)
    x[rng.random((B, D)) < 0.15] = 0.0
    x.flat[rng.integers(0, B * D, max(B * D // 50, 1))] = np.floor(rng.uniform(top / 2, top, max(B * D // 50, 1)))
    rho = rng.uniform(-2.0, 3.0, size=D)
    return x.astype(np.float32), rho.astype(np.float32)


def saturated_batch(B, D, seed=9):
    """The saturated case's batch: zeros, small counts and values up to 1e4; rho cycling through -5, 0, 8."""
    rng = np.random.default_rng(seed)
    x = np.floor(np.exp(rng.uniform(0.0, math.log(1e4), (B, D))))
    x[rng.random((B, D)) < 0.3] = 0.0
    x[0, 0], x[B - 1, D - 1] = 1e4, 0.0
    rho = np.array([-5.0, 0.0, 8.0])[np.arange(D) % 3]
    return x.astype(np.float32), rho.astype(np.float32)


# ---- the cases of tests/test_count.py
@dataclasses.dataclass(frozen=True)
class Case:
    mname: str
    d: object
    B: int


def _dims(mname, D, S):
    K = 1 if mname == "vae" else 3
    return O.Dims(D=D, L=8, K=K, hidden=(64,), S=S)


# B in {32, 5}: 32 gives the 32 x 32 configuration an interior row tile, 5 forces the edge path; D in {128, 100, 13}: interior,
# the last column tile with D % 4 == 0, the element path; S in {1, 3}, alternating so that each meets each B and each D
SHAPES = [(B, D, 1 if (i + j) % 2 == 0 else 3) for i, B in enumerate((32, 5)) for j, D in enumerate((128, 100, 13))]
CASES = {f"{m}-b{B}-d{D}-s{S}": Case(m, _dims(m, D, S), B) for m in ("vae", "vae_gmp", "gmvae") for B, D, S in SHAPES}
VARIANTS = [(n, k) for n in CASES for k in KINDS]


def pad4(n):
    return (n + 3) // 4 * 4


def with_rho(flat, rho32, D):
    tailp = np.zeros(pad4(D), np.float32)
    tailp[:D] = rho32
    return np.concatenate([flat, tailp])


def setup(name, kind, seed=0, saturated=False):
    """(model id, Dims, p as the device sees it, flat fp32 -- rho appended as the layout's last entry under the negative
    binomial --, x float32, eps, u, rho float64 or None).  saturated: the decoder's last layer scaled so that lambda spans about
    +-30, saturated_batch's x and rho."""
    c = CASES[name]
    model = O.MODEL_NAMES[c.mname]
    d = c.d
    rng = np.random.default_rng(seed)
    p = O.init_params(model, d, rng)
    _, eps, u = O.make_inputs(d, c.B, model)
    u = u if model == O.MODEL_GMVAE else None
    x, rho32 = saturated_batch(c.B, d.D) if saturated else count_batch(c.B, d.D)
    if saturated:
        last = f"decoder_fcnet/linear_{len(d.hidden)}/w"
        lam0 = loss_and_grads(model, d, p, x, eps, u, "poisson")[0]["lam"]
        p[last] = p[last] * (30.0 / np.abs(lam0).max())
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    rho = None
    if kind == "nb":
        flat = with_rho(flat, rho32, d.D)
        rho = rho32.astype(np.float64)
    return model, d, p32, flat, x, eps, u, rho
