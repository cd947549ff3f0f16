"""fp64 statement of gmvae_refine (include/gmvae_hip.h; csrc/refine.hpp): per-example refinement of q(z|x) -- stochastic-gradient
ascent on one example's own ELBO over phi = (m, s) of a local Gaussian q_phi(z) = N(m, diag e^{2 s}) (Cremer, Li & Duvenaud 2018),
then the ELBO and the importance-weighted bound of the start and of the refined phi* on common noise.  Test infrastructure only.

  target: log p(x, z) = log p(z) + log p(x|z): ais_ref.prior_table (y summed out) and ais_ref.log_lik, imported, not restated;
  start: (mu_0, sigma_0) [B, 2 L], s_0 = ln sigma_0 held in fp32 like every later s: phi_0 is evaluated at e^{s_0};
  step t: z_s = m + e^s eps_s, g_s = grad_z log p(x, z_s); L-hat_t = 1/S sum_s log p(x, z_s) + sum_l s_l + L/2 (1 + ln 2 pi);
    dm = 1/S sum_s g_s, ds = 1/S sum_s g_s e^s eps_s + 1; one ASCENT step of adam_ref.predict on the 2 L parameters (the gradient
    handed over negated; parameters and moments held in fp32, alpha_t in the fp64-pow form, the example's own count); an example
    whose gradient has an element that is not finite, or, rounded to fp32, is 2^63.5 = 1.3e19 or more in magnitude, skips the
    update (moments and count untouched) -- the device squares the element in fp32 and 2^64 squared is past fp32's largest
    number: its second moment would become inf and freeze the element for good where an fp64 update would move it, so both
    skip, with half a binade to spare; s clamped to
    [-20, 5] after the update;
  evaluation: R rounds of S fresh eps, N = R S; log w = log p(x, z) - log q_phi(z) at phi* and phi_0 on the SAME eps; the ELBO =
    mean log w, the importance-weighted bound = logsumexp log w - ln N, the effective sample size of the N weights at phi*.

Noise is an explicit input: eps [n_steps + R, B S, L], row (b, s) -> b S + s.

refine() also reports, per example, whether an fp32 evaluation can be held to it (the idea of ais_ref's DECIDED chains): an example
is DECIDED if every ReLU pre-activation on its path exceeds 1e-5 in magnitude; at every applied step and element sqrt(v') >= 1e-3
times the example's largest sqrt(v') of that step (below that Adam's ratio m' / sqrt(v') amplifies the gradient's rounding); and no
s lands within 1e-6 of a clamp edge.  Keyword paths for the cases outside the Xavier regime (tests/inference_saturated_cases.py):
rule="clearance" with jitter_seed and ais_ref.well_conditioned, and count="global"."""
import math

import numpy as np

import adam_ref
import ais_ref as A
import oracle as O

F64 = np.float64
LOG_2PI = math.log(2.0 * math.pi)
S_MIN, S_MAX = -20.0, 5.0
G_MAX = np.float32(2.0 ** 63.5)      # kRefineGMax: a gradient element at or above it, as the device holds it in fp32, skips the update
STATS = ("elbo_start", "elbo_refined", "iw_start", "iw_refined", "ess_refined", "updates", "mean_shift", "log_sigma_ratio")


def start_table(model, d, p, x):
    """[B, 2 L] = (mu_0, sigma_0): q(z|x) for the VAE family; for the GMVAE the component at argmax_k q(k|x), lowest index on ties."""
    lw, mu, sg = A.encoder_table(model, d, p, x)
    k = np.argmax(lw, axis=1)
    r = np.arange(lw.shape[0])
    return np.concatenate([mu[r, k], sg[r, k]], axis=1)


class Joint:
    """log p(x, z), its gradient in z and the row's smallest |ReLU pre-activation|, rows example-major with S rows per example."""

    def __init__(self, model, d, p, x, S):
        self.d = d
        self.p = {k: np.asarray(v, F64) for k, v in p.items()}
        self.xr = np.repeat(np.asarray(x).astype(F64), S, axis=0)
        self.prior = A.prior_table(model, d, self.p)

    def __call__(self, z):
        with np.errstate(all="ignore"):
            vp, gp = A.mixture(z, *self.prior)
            vx, gx, margin = A.log_lik(self.d, self.p, self.xr, z)
        return vp + vx, gp + gx, margin


def elbo_and_grad(joint, m, s, e):
    """L-hat [B], (dm, ds) [B, L] each, the smallest ReLU margin [B]; m, s [B, L] (fp64), e [B, S, L]."""
    B, S, L = e.shape
    with np.errstate(all="ignore"):
        sg = np.exp(s)
        z = (m[:, None, :] + sg[:, None, :] * e).reshape(B * S, L)
        val, g, margin = joint(z)
        g = g.reshape(B, S, L)
        lh = val.reshape(B, S).mean(axis=1) + s.sum(axis=1) + 0.5 * L * (1.0 + LOG_2PI)
        return lh, g.mean(axis=1), (g * sg[:, None, :] * e).mean(axis=1) + 1.0, margin.reshape(B, S).min(axis=1)


def log_weights(joint, m, sg, ls, e):
    """log w [B, S] = log p(x, z) - log q(z) at z = m + sg e (ls = ln sg), and the ReLU margin [B]."""
    B, S, L = e.shape
    with np.errstate(all="ignore"):
        z = (m[:, None, :] + sg[:, None, :] * e).reshape(B * S, L)
        val, _, margin = joint(z)
        lq = -ls.sum(axis=1)[:, None] - 0.5 * L * LOG_2PI - 0.5 * (e * e).sum(axis=2)
        return val.reshape(B, S) - lq, margin.reshape(B, S).min(axis=1)


def refine(model, d, p, x, start, n_steps, S, R, lr, b1, b2, adam_eps, eps, rule="sqrt_v", jitter_seed=None, count="own"):
    """Returns dict(phi [B, 2 L] = (m*, sigma*), trace [n_steps, B], stats [B, 8] (STATS), bounds = stats[:, :4], tail [8],
    decided [B] bool, logw_start, logw_refined [B, R S], grads [n_steps, B, 2 L], clamped [B, 2] = the updates of the example
    that were clipped at S_MIN, at S_MAX).
    rule: "sqrt_v" -- DECIDED as the module states it; "clearance" -- the ReLU margin and the clamp clearance alone, for the
    regimes whose gradients span too many orders for the sqrt(v') rule to hold on any example: the caller then asks
    ais_ref.well_conditioned of a second run as well.
    jitter_seed: the gradient each step consumes is multiplied elementwise by 1 + 2^-20 r, r = +-1 from
    default_rng(jitter_seed): that second run.
    count: "own" -- alpha_t from the example's own count of applied updates, as the device does; "global" -- from the step index
    t + 1, the mistake tests/test_inference_saturated_cpu.py shows the own-count case can see."""
    jrng = None if jitter_seed is None else np.random.default_rng(jitter_seed)
    B, L = np.asarray(x).shape[0], d.L
    eps = np.asarray(eps, F64).reshape(n_steps + R, B, S, L)
    start = np.asarray(start, np.float32)
    mu0, sg0 = start[:, :L].astype(F64), start[:, L:].astype(F64)
    with np.errstate(all="ignore"):
        ls0 = np.log(sg0).astype(np.float32).astype(F64)                     # s_0 = ln sigma_0 as the ascent holds it: in fp32
        sg0e = np.exp(ls0)
    joint = Joint(model, d, p, x, S)
    par = np.concatenate([mu0, ls0], axis=1).astype(np.float32)              # m, s: held in fp32
    am, av = np.zeros((B, 2 * L), np.float32), np.zeros((B, 2 * L), np.float32)
    cnt = np.zeros(B, np.int64)
    decided = np.ones(B, bool)
    trace = np.zeros((n_steps, B))
    grads, clamped = np.zeros((n_steps, B, 2 * L)), np.zeros((B, 2), np.int64)
    for t in range(n_steps):
        p64 = par.astype(F64)
        lh, dm, ds, margin = elbo_and_grad(joint, p64[:, :L], p64[:, L:], eps[t])
        trace[t] = lh
        grad = np.concatenate([dm, ds], axis=1)
        if jrng is not None:
            grad = grad * (1.0 + 2.0 ** -20 * jrng.choice([-1.0, 1.0], size=grad.shape))
        grads[t] = grad
        with np.errstate(all="ignore"):
            ok = (np.abs(grad.astype(np.float32)) < G_MAX).all(axis=1)           # (a NaN compares false)
            step_t = (cnt + 1)[:, None] if count == "own" else t + 1
            p2, m2, v2, _ = adam_ref.predict(par, am, av, -grad, 1, step_t, lr, b1, b2, adam_eps)
            sv = np.sqrt(v2)
            ratio = (sv >= 1e-3 * sv.max(axis=1, keepdims=True)).all(axis=1) if rule == "sqrt_v" else True
            decided &= ~ok | ((margin > 1e-5) & ratio &
                              (np.abs(p2[:, L:] - S_MIN) > 1e-6).all(axis=1) & (np.abs(p2[:, L:] - S_MAX) > 1e-6).all(axis=1))
            clamped[:, 0] += ok & (p2[:, L:] < S_MIN).any(axis=1)
            clamped[:, 1] += ok & (p2[:, L:] > S_MAX).any(axis=1)
            p2[:, L:] = np.clip(p2[:, L:], S_MIN, S_MAX)
        o = ok[:, None]
        with np.errstate(all="ignore"):                                          # (a skipped example's p2, m2, v2 are not used)
            par = np.where(o, p2.astype(np.float32), par)
            am, av = np.where(o, m2.astype(np.float32), am), np.where(o, v2.astype(np.float32), av)
        cnt = cnt + ok
    m1, ls1 = par[:, :L].astype(F64), par[:, L:].astype(F64)
    with np.errstate(all="ignore"):
        sg1 = np.exp(ls1)
    lw0, lw1 = [], []
    for r in range(R):
        e = eps[n_steps + r]
        w1, g1 = log_weights(joint, m1, sg1, ls1, e)
        w0, g0 = log_weights(joint, mu0, sg0e, ls0, e)
        decided &= (g1 > 1e-5) & (g0 > 1e-5)
        lw0.append(w0); lw1.append(w1)
    lw0, lw1 = np.concatenate(lw0, axis=1), np.concatenate(lw1, axis=1)          # [B, N]
    N = R * S

    def bounds(lw):
        with np.errstate(all="ignore"):
            mx = lw.max(axis=1, keepdims=True)
            w = np.exp(lw - mx)
            return lw.mean(axis=1), mx[:, 0] + np.log(w.sum(axis=1)) - math.log(N), w.sum(axis=1) ** 2 / (w * w).sum(axis=1)

    e0, i0, _ = bounds(lw0)
    e1, i1, ess = bounds(lw1)
    with np.errstate(all="ignore"):
        stats = np.stack([e0, e1, i0, i1, ess, cnt.astype(F64), (np.abs(m1 - mu0) / sg0).mean(axis=1), (ls1 - ls0).mean(axis=1)], axis=1)
    tail = np.array([e0.sum(), e1.sum(), i0.sum(), i1.sum(), B, 0, 0, 0], F64)
    return dict(phi=np.concatenate([m1, sg1], axis=1), trace=trace, stats=stats, bounds=stats[:, :4], tail=tail, decided=decided,
                logw_start=lw0, logw_refined=lw1, grads=grads, clamped=clamped)


# ------------------------------------------------------------------------------------------------------- the parity cases
# (model, act, D, L, K, hidden, B, S[, n_steps]): the small shapes of test_ais.py's CASES -- D = 23 takes a vector gen_bias --; B S
# rows make one panel of 16 hold several examples and, where S < 16, leave another ragged; then the gates' upper corner, the
# reference's default sizes, and every size 1.  Shared by test_refine_cpu.py (the undecided shares) and test_refine.py (parity).
PARITY = dict(n_steps=8, lr=0.05, R=2, betas=(0.9, 0.999), adam_eps=1e-8, seed=7, step=3)
CASES = [
    ("gmvae", "relu", 24, 3, 4, (16,), 5, 4),
    ("gmvae", "tanh", 23, 5, 3, (12, 20), 19, 1),
    ("gmvae", "relu", 23, 3, 4, (), 3, 8),
    ("gmvae", "elu", 23, 5, 3, (16,), 2, 16),
    ("vae", "relu", 23, 5, 1, (12, 20), 2, 16),
    ("vae", "tanh", 24, 3, 1, (16,), 5, 4),
    ("vae", "sigmoid", 24, 5, 1, (), 19, 1),
    ("vae_gmp", "relu", 24, 5, 3, (12, 20), 19, 1),
    ("vae_gmp", "sigmoid", 24, 3, 4, (12, 20), 5, 4),
    ("vae_gmp", "tanh", 23, 3, 4, (16,), 6, 2),
    ("vae_gmp", "relu", 24, 3, 4, (), 2, 16),
    ("gmvae", "tanh", 23, 128, 64, (512, 512, 512), 2, 2, 2),
    ("gmvae", "relu", 784, 64, 10, (64,), 5, 4),
    ("vae_gmp", "tanh", 1, 1, 1, (1,), 5, 4),
]
# (data seed, weight scale) of the two wide cases.  With 128 and 256 parameters per example and weights at twice Xavier the first
# steps' sqrt(v') criterion -- d s is near 1 where d m runs into the hundreds -- leaves most examples undecided on every seed
# tried, so these two run at plain Xavier, their seeds chosen for the statement alone to stay within the cap (the shares are in
# profiles/refine_notes.md).  Every other case: seed 2000 + its index, scale 2.
DATA_SEED = {("gmvae", "tanh", 23, 128, 64, (512, 512, 512), 2, 2, 2): (4129, 1.0),
             ("gmvae", "relu", 784, 64, 10, (64,), 5, 4): (4223, 1.0)}
MODELS = {"vae": O.MODEL_VAE, "vae_gmp": O.MODEL_VAE_GMP, "gmvae": O.MODEL_GMVAE}
cid = lambda c: "-".join(str(v).replace(" ", "") for v in c)


def make(model, d, B, seed, scale=2.0):
    """Xavier weights times `scale`, small random biases, x ~ Bernoulli(1/2): (params fp32-exact, flat, x) -- test_ais.make."""
    rng = np.random.default_rng(seed)
    p = {k: scale * v for k, v in O.init_params(model, d, rng).items()}
    for k in p:
        if k.endswith("/b"):
            p[k] = 0.1 * rng.standard_normal(p[k].shape)
    flat = O.pack(model, d, p)
    p = {k: v.astype(F64) for k, v in O.unpack(model, d, flat).items()}
    x = (rng.random((B, d.D)) < 0.5).astype(np.uint8)
    return p, flat, x


def case_inputs(case):
    """(model id, dims, params, flat, x, start fp32, S, n_steps) of a parity case."""
    name, act, D, Lz, K, hidden, B, S = case[:8]
    n_steps = case[8] if len(case) > 8 else PARITY["n_steps"]
    model = MODELS[name]
    d = O.Dims(D=D, L=Lz, K=K, hidden=hidden, act=act, gen_bias_init=np.linspace(-0.5, 0.5, D).astype(np.float32) if D == 23 else 0.1)
    p, flat, x = make(model, d, B, *DATA_SEED.get(case, (2000 + CASES.index(case), 2.0)))
    return model, d, p, flat, x, start_table(model, d, p, x).astype(np.float32), S, n_steps


def run_case(case, eps):
    """The statement on a parity case with the noise eps [n_steps + R, B S, L]."""
    model, d, p, flat, x, start, S, n_steps = case_inputs(case)
    P = PARITY
    return refine(model, d, p, x, start, n_steps, S, P["R"], P["lr"], *P["betas"], P["adam_eps"], eps)
