"""fp64 statement of gmvae_ais (include/gmvae_hip.h; csrc/ais.hpp): log p(x) by annealed importance sampling with Hamiltonian
Monte Carlo transitions (Neal 2001; Wu, Burda, Salakhutdinov & Grosse 2017), on the generative model of oracle.forward.

  prior p(z): a K-component diagonal mixture table (ln pi_k, mu_k, sigma_k) -- prior_table;
  base r_b(z): the prior, or the example's inference mixture as a table of the same form -- encoder_table;
  log p(x|z): the Bernoulli term of oracle.forward (decoder MLP, gen_bias_init scalar or vector, any act), the activation's
  derivative taken from the activation (oracle._dact: ReLU' = 0 at a pre-activation <= 0);
  f_t = r^(1 - beta_t) (p p(x|.))^beta_t; with the prior as the base: p(z) p(x|z)^beta_t, the prior evaluated once.

Noise is an explicit input: eps [T + 1, B C, L], u [T + 1, B C]; row (b, c) -> b C + c; t = 0 is the start (u picks the component
by inverse CDF, z_0 = mu_k + sigma_k eps), t >= 1 the transition at beta_t (eps the momentum, u the accept uniform).

ais() also reports, per chain, whether an fp32 evaluation can be held to its accept sequence: a chain is DECIDED if every
|ln u - dH| exceeds 1e-4 (|H_old| + |H_new|) + 1e-6, every ReLU pre-activation along its path exceeds 1e-5 in magnitude, and the
component pick is not within 1e-6 of a CDF edge.  Two keyword paths serve the cases outside the Xavier regime
(tests/inference_saturated_cases.py): nonfinite_is_decided, and jitter_seed with well_conditioned() -- a conditioning measure from
the statement alone, for where the fixed margins above say nothing."""
import math

import numpy as np

import oracle as O
from oracle.gmvae_oracle import _act, _dact, _log_softmax, _normal_head, _mlp_fwd

LOG_2PI = math.log(2.0 * math.pi)
STEP_MIN, STEP_MAX = 1e-4, 1.0
F64 = np.float64


def schedule(kind, T):
    """beta_0 .. beta_T: "linear", or "sigmoid": (s(4 (2 t / T - 1)) - s(-4)) / (s(4) - s(-4)) (Wu et al. 2017)."""
    t = np.arange(T + 1, dtype=F64)
    if kind == "linear":
        b = t / T
    elif kind == "sigmoid":
        s = lambda v: 1.0 / (1.0 + np.exp(-v))
        b = (s(4.0 * (2.0 * t / T - 1.0)) - s(-4.0)) / (s(4.0) - s(-4.0))
    else:
        raise ValueError(kind)
    b[0], b[-1] = 0.0, 1.0
    return b


def prior_table(model, d, p):
    """(ln pi [K], mu [K, L], sigma [K, L]) of the model's prior."""
    p = {k: np.asarray(v, F64) for k, v in p.items()}
    if model == O.MODEL_VAE:
        return np.zeros(1), np.zeros((1, d.L)), np.ones((1, d.L))
    if model == O.MODEL_VAE_GMP:
        return _log_softmax(p["mixture_logits"]), p["loc"], O.softplus(p["raw_scale_diag"])
    pp = np.eye(d.K) @ p["prior_gmm_fcnet/linear_0/w"] + p["prior_gmm_fcnet/linear_0/b"]
    mu, sig, _ = _normal_head(pp, d.L, F64(d.raw_sigma_bias), F64(d.sigma_min))
    return np.full(d.K, -math.log(d.K)), mu, sig


def encoder_table(model, d, p, x):
    """(ln w [B, Kb], mu [B, Kb, L], sigma [B, Kb, L]) of the inference mixture: one Gaussian q(z|x) for the VAE family,
    sum_k q(k|x) q(z|x, e_k) for the GMVAE."""
    p = {k: np.asarray(v, F64) for k, v in p.items()}
    xf = np.asarray(x).astype(F64)
    B, nl = xf.shape[0], len(d.hidden) + 1
    c, smin = F64(d.raw_sigma_bias), F64(d.sigma_min)
    if model != O.MODEL_GMVAE:
        qp, _ = _mlp_fwd(p, "encoder", nl, xf, act=d.act)
        mu, sig, _ = _normal_head(qp, d.L, c, smin)
        return np.zeros((B, 1)), mu[:, None, :], sig[:, None, :]
    logits, _ = _mlp_fwd(p, "encoder_y", nl, xf, act=d.act)
    xr = np.repeat(xf, d.K, axis=0)
    y = np.tile(np.eye(d.K), (B, 1))
    qp, _ = _mlp_fwd(p, "encoder_gmm", nl, np.concatenate([xr, y], axis=1), act=d.act)
    mu, sig, _ = _normal_head(qp, d.L, c, smin)
    return _log_softmax(logits), mu.reshape(B, d.K, d.L), sig.reshape(B, d.K, d.L)


def mixture(z, lnw, mu, sig):
    """ln sum_k w_k N(z; mu_k, sigma_k) and its gradient in z.  z [R, L]; the table per row ([R, K], [R, K, L]) or shared
    ([K], [K, L])."""
    if lnw.ndim == 1:
        lnw, mu, sig = lnw[None], mu[None], sig[None]
    t = (z[:, None, :] - mu) / sig
    comp = lnw + (-0.5 * t * t - 0.5 * LOG_2PI).sum(axis=2) - np.log(sig).sum(axis=2)
    m = comp.max(axis=1, keepdims=True)
    val = (m + np.log(np.exp(comp - m).sum(axis=1, keepdims=True)))[:, 0]
    resp = np.exp(comp - val[:, None])
    return val, -(resp[:, :, None] * t / sig).sum(axis=1)


def log_lik(d, p, xr, z):
    """log p(x|z) per row, its gradient in z, and the smallest |ReLU pre-activation| of the row (inf without ReLU layers)."""
    nl = len(d.hidden) + 1
    pres = []
    lam, hs = _mlp_fwd(p, "decoder", nl, z, pres, act=d.act)
    lam = lam + np.asarray(d.gen_bias_init, F64)
    val = (xr * lam - O.softplus(lam)).sum(axis=1)
    g = xr - O.sigmoid(lam)
    for i in reversed(range(nl)):
        g = g @ p[f"decoder_fcnet/linear_{i}/w"].T
        if i > 0:
            g = g * _dact(hs[i], d.act)
    margin = np.full(z.shape[0], np.inf)
    if d.act == "relu":
        for pre, _ in pres:
            margin = np.minimum(margin, np.abs(pre).min(axis=1))
    return val, g, margin


class Target:
    """The two parts (A, B) of log f_t = cA A + cB B and log w's increment, for a batch of chains (row r of example r // C)."""

    def __init__(self, model, d, p, x, C, init, base=None):
        self.d = d
        self.p = {k: np.asarray(v, F64) for k, v in p.items()}
        self.xr = np.repeat(np.asarray(x).astype(F64), C, axis=0)
        self.prior = prior_table(model, d, self.p)
        self.enc = init == "encoder"
        if init not in ("prior", "encoder"):
            raise ValueError(init)
        if self.enc:
            lw, mu, sg = base if base is not None else encoder_table(model, d, self.p, x)
            self.base = tuple(np.repeat(np.asarray(a, F64), C, axis=0) for a in (lw, mu, sg))

    def coef(self, beta):
        return ((1.0 - beta) if self.enc else 1.0), beta

    def parts(self, z):
        """A, B, grad A, grad B, ReLU margin."""
        vx, gx, margin = log_lik(self.d, self.p, self.xr, z)
        vp, gp = mixture(z, *self.prior)
        if not self.enc:
            return vp, vx, gp, gx, margin
        vr, gr = mixture(z, *self.base)
        return vr, vp + vx, gr, gp + gx, margin

    def dlogw(self, vA, vB):
        return vB - vA if self.enc else vB

    def start(self, eps, u):
        """z_0 and the distance of u to the nearest CDF edge."""
        R = eps.shape[0]
        lw, mu, sg = self.base if self.enc else tuple(np.broadcast_to(a[None], (R,) + a.shape) for a in self.prior)
        cdf = np.cumsum(np.exp(lw), axis=1)
        K = cdf.shape[1]
        k = np.minimum((u[:, None] >= cdf).sum(axis=1), K - 1)
        edge = np.abs(u[:, None] - cdf[:, :K - 1]).min(axis=1) if K > 1 else np.full(R, np.inf)
        rows = np.arange(R)
        return mu[rows, k] + sg[rows, k] * eps, edge


def ais(model, d, p, x, betas, C, n_leapfrog, step0, eps, u, init="prior", step_up=1.02, step_down=0.96, base=None,
        nonfinite_is_decided=False, jitter_seed=None, z0_fp32=False):
    """The chains of every example of x.  Returns dict(logw [B, C], bound [B], stats [B, 4], z [B C, L], tail [8],
    accepts [T, B C] bool, decided [B C] bool, steps [B C], h_new [T, B C], z0 [B C, L], clips [B C, 2] = the number of
    transitions whose step size the clip to STEP_MIN, to STEP_MAX changed).
    nonfinite_is_decided: a transition whose fp64 h_new is not finite counts as a decided reject -- fp32 overflows no later than
    fp64, and a NaN of inf - inf is a NaN in both --; the ReLU margin is then not asked of that transition's path.
    jitter_seed: every gradient a transition consumes is multiplied elementwise by 1 + 2^-20 r, r = +-1 from
    default_rng(jitter_seed) -- a few fp32 ulps --, and the start z_0 is rounded to fp32, the format a device holds the chain's
    state in (a base sigma below an ulp of mu, 6e-8 |mu|, is not resolved by such a state: log r(z_0) then depends on the
    rounding by up to eps^2 / 2 per dimension): the second run of well_conditioned().
    z0_fp32: the first run starts from z_0 rounded to fp32 as well -- the statement of a chain whose state is fp32 from the start,
    for a case whose base is that narrow."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):      # (a proposal that is not finite is a case here)
        return _ais(model, d, p, x, betas, C, n_leapfrog, step0, eps, u, init, step_up, step_down, base, nonfinite_is_decided,
                    jitter_seed, z0_fp32)


def _ais(model, d, p, x, betas, C, n_leapfrog, step0, eps, u, init, step_up, step_down, base, nonfinite_is_decided, jitter_seed,
         z0_fp32):
    jit = lambda g: g
    if jitter_seed is not None:
        jrng = np.random.default_rng(jitter_seed)
        jit = lambda g: g * (1.0 + 2.0 ** -20 * jrng.choice([-1.0, 1.0], size=g.shape))
    betas = np.asarray(betas, F64)
    T = len(betas) - 1
    B = np.asarray(x).shape[0]
    R = B * C
    eps = np.asarray(eps, F64).reshape(T + 1, R, d.L)
    u = np.asarray(u, F64).reshape(T + 1, R)
    tg = Target(model, d, p, x, C, init, base)
    z, edge = tg.start(eps[0], u[0])
    if jitter_seed is not None or z0_fp32:
        z = z.astype(np.float32).astype(F64)
    z0 = z.copy()
    decided = edge > 1e-6
    vA, vB, gA, gB, margin = tg.parts(z)
    gA, gB = jit(gA), jit(gB)
    decided &= margin > 1e-5
    logw = np.zeros(R)
    step = np.full(R, min(max(float(step0), STEP_MIN), STEP_MAX))
    accepts = np.zeros((T, R), bool)
    h_news, clips = np.zeros((T, R)), np.zeros((R, 2), np.int64)
    for t in range(1, T + 1):
        logw = logw + (betas[t] - betas[t - 1]) * tg.dlogw(vA, vB)
        cA, cB = tg.coef(betas[t])
        mom = eps[t].copy()
        h_old = -(cA * vA + cB * vB) + 0.5 * (mom * mom).sum(axis=1)
        e = step[:, None]
        zn = z.copy()
        mom = mom + 0.5 * e * (cA * gA + cB * gB)
        path_ok = np.ones(R, bool)
        for i in range(1, n_leapfrog + 1):
            zn = zn + e * mom
            nA, nB, ngA, ngB, margin = tg.parts(zn)
            ngA, ngB = jit(ngA), jit(ngB)
            path_ok &= margin > 1e-5
            mom = mom + (e if i < n_leapfrog else 0.5 * e) * (cA * ngA + cB * ngB)
        h_new = -(cA * nA + cB * nB) + 0.5 * (mom * mom).sum(axis=1)
        with np.errstate(invalid="ignore"):
            dh = h_old - h_new
            acc = np.isfinite(h_new) & (np.log(u[t]) < dh)
            clear = path_ok & np.isfinite(h_new) & (np.abs(np.log(u[t]) - dh) > 1e-4 * (np.abs(h_old) + np.abs(h_new)) + 1e-6)
            decided &= (clear | ~np.isfinite(h_new)) if nonfinite_is_decided else clear
        accepts[t - 1] = acc
        h_news[t - 1] = h_new
        a = acc[:, None]
        z, gA, gB = np.where(a, zn, z), np.where(a, ngA, gA), np.where(a, ngB, gB)
        vA, vB = np.where(acc, nA, vA), np.where(acc, nB, vB)
        raw = step * np.where(acc, step_up, step_down)
        clips[:, 0] += raw < STEP_MIN
        clips[:, 1] += raw > STEP_MAX
        step = np.clip(raw, STEP_MIN, STEP_MAX)
    lw = logw.reshape(B, C)
    m = lw.max(axis=1, keepdims=True)
    w = np.exp(lw - m)
    bound = m[:, 0] + np.log(w.sum(axis=1)) - math.log(C)
    ess = w.sum(axis=1) ** 2 / (w * w).sum(axis=1)
    rate = accepts.reshape(T, B, C).mean(axis=(0, 2))
    stats = np.stack([bound, ess, rate, step.reshape(B, C).mean(axis=1)], axis=1)
    tail = np.array([-bound.sum(), ess.sum(), rate.sum(), stats[:, 3].sum(), B, 0, 0, 0], F64)
    return dict(logw=lw, bound=bound, stats=stats, z=z, tail=tail, accepts=accepts, decided=decided, steps=step,
                h_new=h_news, z0=z0, clips=clips)


def well_conditioned(ref, jittered, keys=("logw", "z"), rel=1e-5):
    """[rows] bool from two runs of a statement, the second with jitter_seed set: the accept sequence (ais) or the applied count
    (refine_ref.refine) is unchanged and every output named moves by at most rel max(1, |.|) -- a tenth of the project's 1e-4
    gate, which so keeps a tenfold margin over what rounding of a few fp32 ulps in the gradients does to the reference itself.
    An output that is not finite in both runs alike counts as unmoved."""
    n = ref["decided"].shape[0]
    if "accepts" in ref:
        ok = (ref["accepts"] == jittered["accepts"]).all(axis=0)
    else:
        ok = ref["stats"][:, 5] == jittered["stats"][:, 5]
    for k in keys:
        a, b = np.asarray(ref[k], F64), np.asarray(jittered[k], F64)
        if k == "trace":                                   # [n_steps, B]
            a, b = a.T, b.T
        a, b = a.reshape(n, -1), b.reshape(n, -1)
        with np.errstate(invalid="ignore"):
            same = np.abs(a - b) <= rel * np.maximum(1.0, np.abs(a))
            same |= ~np.isfinite(a) & ~np.isfinite(b) & ((a == b) | (np.isnan(a) & np.isnan(b)))
        ok &= same.all(axis=1)
    return ok


def bound_stderr(logw):
    """Delta-method standard error of logsumexp_c logw - ln C from the C weights of each row of logw [B, C]."""
    lw = np.asarray(logw, F64)
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    return w.std(axis=1, ddof=1) / (w.mean(axis=1) * math.sqrt(lw.shape[1]))


def quadrature_log_px(model, d, p, x, lim=8.0, n=801):
    """log p(x_b) of an L = 2 model by the trapezoid rule on an n x n grid over [-lim, lim]^2."""
    assert d.L == 2
    p = {k: np.asarray(v, F64) for k, v in p.items()}
    g = np.linspace(-lim, lim, n)
    h = g[1] - g[0]
    zz = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    wq = np.ones(n); wq[0] = wq[-1] = 0.5
    lnq = np.log(np.outer(wq, wq).reshape(-1)) + 2.0 * math.log(h)
    vp, _ = mixture(zz, *prior_table(model, d, p))
    nl = len(d.hidden) + 1
    lam, _ = _mlp_fwd(p, "decoder", nl, zz, act=d.act)
    lam = lam + np.asarray(d.gen_bias_init, F64)
    sp = O.softplus(lam).sum(axis=1)
    out = []
    for xb in np.asarray(x).astype(F64):
        v = lam @ xb - sp + vp + lnq
        m = v.max()
        out.append(m + math.log(np.exp(v - m).sum()))
    return np.array(out)
