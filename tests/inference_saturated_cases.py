"""The cases of tests/test_inference_saturated*.py: gmvae_ais (csrc/ais.hpp) and gmvae_refine (csrc/refine.hpp) OUTSIDE the Xavier
regime -- test infrastructure, a plain module like saturated_cases.py.

Parameters are test_saturated.saturate's in saturated_cases.REGIMES (trained: sigma of the q head from 3e-4 to 8, the prior's from
0.13 to 2.1, largest |lambda| 60; diverging: both from 2e-9 to 20), encoder_y's logits at +-15; the VAE_GMP's mixture_logits are
scaled on top so that its smallest pi is below 1e-30 (one dominant component in the inverse-CDF pick and in ln pi).  They go through
oracle.pack(..., float32) and oracle.unpack, so the statement sees the device's bits.

Which chains or examples a case holds the device to (`kept`) is decided on the fp64 statement alone:
  AIS          DECIDED (ais_ref.ais, with nonfinite_is_decided where the case is about a proposal that is not finite) AND
               well-conditioned (ais_ref.well_conditioned against a second run with jittered gradients and an fp32 start);
  refinement   trained: DECIDED as refine_ref states it; diverging, and the cases that start on a clamp or past the skip bound:
               well-conditioned, the ReLU margin and the clamp clearance (rule="clearance") -- there the gradients span 17 orders
               of magnitude and the sqrt(v') rule fails on every example.
A case may leave out at most 10 % (CAP) -- a condition on the table below, asserted by tests/test_inference_saturated_cpu.py on the
restated noise and again by tests/test_inference_saturated.py on the device's own draws.  A case that missed it got another seed,
T or step0 HERE, with the reason next to it; the figures are in profiles/inference_saturated_notes.md.

Statements on the restated noise are computed once (ais_cpu, refine_cpu), shared, and left unchanged."""
import dataclasses

import numpy as np

import ais_ref as A
import oracle as O
import refine_ref as RF
from saturated_cases import REGIMES
from test_saturated import saturate

CAP = 0.10
SEED, STEP = 7, 3                  # the Philox key of both entry points' tests (test_ais.device_ais, refine_ref.PARITY)
JITTER_SEED = 20261020
ADAM = dict(lr=0.05, betas=(0.9, 0.999), adam_eps=1e-8, R=2)      # refine_ref.PARITY's
INF = float("inf")


@dataclasses.dataclass(frozen=True)
class Ais:
    mname: str
    init: str                     # prior | encoder
    act: str
    D: int
    L: int
    K: int
    hidden: tuple
    B: int
    C: int
    regime: str
    T: int = 8
    leap: int = 3
    step0: float = 0.02
    up: float = 1.02
    down: float = 0.96
    seed: int = 0
    kind: str = "parity"          # parity | clip_low | clip_high | inf_eps | overflow
    inject: tuple = ()            # (t, chain): eps[t, chain, :] = inf
    z0_fp32: bool = False         # the statement starts from z_0 rounded to fp32 (ais_ref.ais)


@dataclasses.dataclass(frozen=True)
class Refine:
    mname: str
    act: str
    D: int
    L: int
    K: int
    hidden: tuple
    B: int
    S: int
    regime: str
    n_steps: int = 8
    seed: int = 0
    kind: str = "parity"          # parity | own_count | clamp | seam
    rule: str = None              # None: refine_rule's choice by regime and kind
    inject: tuple = ()            # (t, example): eps[t, rows of the example, :] = inf


# ------------------------------------------------------------------------------------------------------------------ AIS
# Shapes: D = 24 and 23 (a vector gen_bias_init), L = 5 and 3, K = 4 and 3, hidden (16,) and (12, 20), relu and tanh, the three
# models, both bases; B = 4 x C = 16 (full 16-row panels) and B = 3 x C = 5 (one ragged panel).
# step0 of the `trained` cases: the largest of 0.3, 0.15, 0.08, 0.04, ... at which the statement leaves at most CAP out with room
# to spare and accepts some but not all proposals (at 0.02 and below the prior-based ones accept everything and the accept margin
# 1e-4 (|H_old| + |H_new|), |H| near 1000, leaves up to a quarter of the encoder-based ones undecided).  From the encoder the
# chains accept about one transition in eight: sigma of the base runs down to 3e-4, so a leapfrog step of any such size is
# unstable until beta_t takes the base out of the target.  In `diverging` every proposal is rejected at every step0.
AIS = {
    "trained-gmvae-prior": Ais("gmvae", "prior", "relu", 24, 5, 4, (16,), 4, 16, "trained", step0=0.08),
    "trained-gmvae-encoder": Ais("gmvae", "encoder", "tanh", 23, 3, 3, (12, 20), 3, 5, "trained", step0=0.08),
    "trained-vae-prior": Ais("vae", "prior", "tanh", 24, 3, 1, (16,), 3, 5, "trained", step0=0.15),
    "trained-vae-encoder": Ais("vae", "encoder", "relu", 23, 5, 1, (12, 20), 4, 16, "trained", step0=0.04),
    "trained-vae_gmp-prior": Ais("vae_gmp", "prior", "relu", 23, 3, 4, (12, 20), 4, 16, "trained", step0=0.15),
    "trained-vae_gmp-encoder": Ais("vae_gmp", "encoder", "tanh", 24, 5, 3, (16,), 3, 5, "trained", step0=0.08),
    "diverging-gmvae-prior": Ais("gmvae", "prior", "tanh", 24, 5, 4, (16,), 3, 5, "diverging"),
    "diverging-gmvae-encoder": Ais("gmvae", "encoder", "relu", 23, 3, 3, (12, 20), 4, 16, "diverging"),
    "diverging-vae_gmp-prior": Ais("vae_gmp", "prior", "tanh", 23, 5, 4, (16,), 4, 16, "diverging"),
    "diverging-vae_gmp-encoder": Ais("vae_gmp", "encoder", "relu", 24, 3, 3, (12, 20), 3, 5, "diverging"),
    # The VAE's prior is N(0, 1), so here log w stays near 1e3 and the gate is not relative to 1e17: the one case that SEES that a
    # base sigma of 3.5e-9 around mu = 0.66 lies below fp32's ulp of z (6e-8).  z_0 = fl(mu + sigma eps) is mu itself and
    # log r(z_0) is off by eps^2 / 2: from the exact z_0 the statement's log w is up to 73 gates from the one started at the
    # rounded z_0, the jittered run leaves out 13 of 15 chains, and the device (measured: 45 gates from the exact start) cannot
    # be held to it.  It is held to the statement of a chain whose state is fp32 from the start (z0_fp32); the mixture-prior cases
    # carry the same rounding under a gate of 1e-4 |log w| = 1e13 (profiles/inference_saturated_notes.md).
    "diverging-vae-encoder": Ais("vae", "encoder", "tanh", 24, 5, 1, (16,), 3, 5, "diverging", z0_fp32=True),
    # the reference's default sizes
    "trained-default-sizes": Ais("gmvae", "prior", "relu", 784, 64, 10, (64,), 2, 16, "trained", T=2, leap=2, step0=0.15),
    # ---- the step-size clips.  Low: every proposal rejected, 2e-4 halved is below kAisStepMin at the first transition.
    "clip-low": Ais("vae_gmp", "encoder", "relu", 24, 3, 3, (12, 20), 3, 5, "diverging", step0=2e-4, down=0.5, kind="clip_low"),
    # High: from the encoder at 0.9 nothing is accepted before the last transition (beta = 1: the base has left the target), where
    # 0.9 0.96^7 1.5 = 1.014 is clipped.  Seed 2: of seeds 0 .. 3 the one whose accepting chains are mostly well-conditioned (3
    # chains accept, 2 of them kept, 1 of 64 left out; seed 0: 6 accept, 1 kept, 5 left out).
    "clip-high": Ais("vae", "encoder", "relu", 23, 5, 1, (12, 20), 4, 16, "trained", step0=0.9, up=1.5, seed=2, kind="clip_high"),
    # ---- a proposal that is not finite.  (a) momenta of inf at transition 3 of chain 3 (a full panel) and chain 18 (the ragged
    # one): B = 4 x C = 5 as test_ais._bits_case.
    "inf-eps": Ais("gmvae", "prior", "relu", 24, 5, 4, (16,), 4, 5, "trained", step0=0.08, kind="inf_eps", inject=((3, 3), (3, 18))),
    # (b) ten leapfrog steps of 1.0 against sigma = 2e-9: H_new is past fp32 on every chain -- NaN in fp64 too from the encoder,
    # finite in fp64 (above 3.4e38) from the VAE_GMP's prior
    "overflow-gmvae-encoder": Ais("gmvae", "encoder", "relu", 23, 3, 3, (12, 20), 4, 16, "diverging", step0=1.0, leap=10,
                                  kind="overflow"),
    "overflow-vae_gmp-prior": Ais("vae_gmp", "prior", "tanh", 23, 5, 4, (16,), 4, 16, "diverging", step0=1.0, leap=10,
                                  kind="overflow"),
}
# the all-reject parity case on the same parameters and noise keys as an overflow case: its z_T is z_0 as well
OVERFLOW_TWIN = {"overflow-gmvae-encoder": "diverging-gmvae-encoder", "overflow-vae_gmp-prior": "diverging-vae_gmp-prior"}


def _key(c):
    return (c.mname, c.act, c.D, c.L, c.K, c.hidden, c.B, c.regime, c.seed, c.kind == "seam")


_PARAMS = {}


def params(c):
    """dict(model, d, p (the fp32 parameters in fp64, unpacked), flat (fp32), x) of a case of either table; cases that differ in
    the sampler's settings alone share it."""
    k = _key(c)
    if k not in _PARAMS:
        model = O.MODEL_NAMES[c.mname]
        d = O.Dims(D=c.D, L=c.L, K=c.K, hidden=c.hidden, act=c.act,
                   gen_bias_init=np.linspace(-0.5, 0.5, c.D).astype(np.float32) if c.D == 23 else 0.1)
        rng = np.random.default_rng(1000 * c.seed + c.B + c.L)
        x, _, _ = O.make_inputs(d, c.B, model, seed_x=100 + c.seed)
        p = saturate(model, d, O.init_params(model, d, rng), rng, x, logit=15.0, **REGIMES[c.regime])
        if model == O.MODEL_VAE_GMP:          # smallest pi below 1e-30: the logits' range stretched to 80 nats
            ml = p["mixture_logits"]
            p["mixture_logits"] = ml * (80.0 / (ml.max() - ml.min()))
        if c.kind == "seam":                  # sigma_k of ONE latent dimension at 2e-9, in every component (one component alone
            p["raw_scale_diag"][:, SEAM_DIM] = np.log(np.expm1(SEAM_SIGMA))      # would only hand z to the others)
        flat = O.pack(model, d, p, np.float32)
        _PARAMS[k] = dict(model=model, d=d, flat=flat, p=O.unpack(model, d, flat.astype(np.float64)), x=x)
    return _PARAMS[k]


def ais_base(c):
    """The caller's base table in fp32 (None from the prior)."""
    if c.init != "encoder":
        return None
    i = params(c)
    return tuple(a.astype(np.float32) for a in A.encoder_table(i["model"], i["d"], i["p"], i["x"]))


def ais_restated_noise(c):
    """oracle.noise at gmvae_ais's keys: eps [T + 1, B C, L], u [T + 1, B C] (Box-Muller restated to a few 1e-6, u to the bit)."""
    n = c.B * c.C
    eu = [O.noise(n, c.L, 1, 0, SEED, STEP * (c.T + 1) + t) for t in range(c.T + 1)]
    return np.stack([e for e, _ in eu]).astype(np.float32), np.stack([u[:, 0] for _, u in eu]).astype(np.float32)


def ais_injected(c, eps):
    """A copy of eps with the case's momenta that are not finite put in."""
    eps = np.array(eps, np.float32)
    for t, chain in c.inject:
        eps[t, chain, :] = INF
    return eps


def ais_run(c, eps, u, step0=None):
    """The statement on a case with the noise given (already injected): ais_ref.ais's dict plus `kept` = DECIDED AND
    well-conditioned, and `well` itself."""
    i = params(c)
    betas = A.schedule("sigmoid", c.T).astype(np.float32).astype(np.float64)
    nf = c.kind in ("inf_eps", "overflow")
    kw = dict(init=c.init, step_up=c.up, step_down=c.down, base=ais_base(c), nonfinite_is_decided=nf, z0_fp32=c.z0_fp32)
    args = (i["model"], i["d"], i["p"], i["x"], betas, c.C, c.leap, c.step0 if step0 is None else step0, eps, u)
    ref = A.ais(*args, **kw)
    ref["well"] = A.well_conditioned(ref, A.ais(*args, jitter_seed=JITTER_SEED, **kw))
    ref["kept"] = ref["decided"] & ref["well"]
    return ref


_AIS_CPU = {}


def ais_cpu(name):
    """The statement of a case on the restated noise -- computed once, shared, left unchanged."""
    if name not in _AIS_CPU:
        c = AIS[name]
        eps, u = ais_restated_noise(c)
        _AIS_CPU[name] = ais_run(c, ais_injected(c, eps), u)
    return _AIS_CPU[name]


# ----------------------------------------------------------------------------------------------------------- refinement
# B = 5 x S = 4 and B = 19 x S = 1: several examples share one 16-row panel and one panel is ragged.
# Seeds: the first of 0, 1, 2, ... at which the statement on the restated noise leaves nobody out (B = 5: CAP allows none) or at
# most one of 19.  At seed 0 the sqrt(v') rule left out 3 of 5, 15 of 19, 1 of 5, 3 of 19 and 1 of 5 of the `trained` cases that
# carry another seed, and the jitter 3 of 5 and 2 of 5 of the two `diverging` S = 4 cases (profiles/inference_saturated_notes.md).
REFINE = {
    "trained-gmvae-s4": Refine("gmvae", "relu", 24, 5, 4, (16,), 5, 4, "trained", seed=2),
    "trained-gmvae-s1": Refine("gmvae", "tanh", 23, 3, 3, (12, 20), 19, 1, "trained", seed=1),
    "trained-vae-s1": Refine("vae", "tanh", 24, 3, 1, (16,), 19, 1, "trained"),
    "trained-vae-s4": Refine("vae", "relu", 23, 5, 1, (12, 20), 5, 4, "trained", seed=3),
    "trained-vae_gmp-s1": Refine("vae_gmp", "relu", 23, 3, 4, (16,), 19, 1, "trained", seed=3),
    "trained-vae_gmp-s4": Refine("vae_gmp", "tanh", 24, 5, 3, (12, 20), 5, 4, "trained", seed=1),
    # (seed 3: three examples meet gradients past the skip bound of 2^63.5 at some steps -- counts 5, 6 and 7 --, so this case
    # holds the own count and the bound on the statement's own gradients as well)
    "diverging-gmvae-s4": Refine("gmvae", "tanh", 24, 5, 4, (16,), 5, 4, "diverging", seed=3),
    "diverging-gmvae-s1": Refine("gmvae", "relu", 23, 3, 3, (12, 20), 19, 1, "diverging"),      # (counts 2 .. 7 likewise)
    "diverging-vae_gmp-s4": Refine("vae_gmp", "relu", 24, 5, 3, (12, 20), 5, 4, "diverging", seed=3),
    "diverging-vae_gmp-s1": Refine("vae_gmp", "tanh", 23, 3, 4, (16,), 19, 1, "diverging"),
    "diverging-vae-s4": Refine("vae", "tanh", 24, 5, 1, (16,), 5, 4, "diverging"),
    # The reference's default sizes.  Under the sqrt(v') rule all 5 examples are undecided on every seed of 0 .. 8: with 128
    # parameters per example, d s near 1 and d m in the thousands, the rule cannot hold (refine_ref.DATA_SEED says the same of its
    # wide cases, which for that reason run at plain Xavier); so this case takes the replacement rule of the diverging ones.
    "trained-default-sizes": Refine("gmvae", "relu", 784, 64, 10, (64,), 5, 4, "trained", n_steps=2, rule="clearance"),
    # ---- the example's own count: example 1 skips steps 2 and 5, example 3 step 0 (its first update is at step 1 with count 1)
    "own-count": Refine("gmvae", "relu", 24, 5, 4, (16,), 5, 4, "trained", seed=2, kind="own_count", inject=((2, 1), (5, 1), (0, 3))),
    # ---- the clamp: sigma_0 = 2e-9 and 200 in two dimensions of every example (clamp_dims).  The lower edge engages in the
    # diverging regime only; seed 3 as above.
    "clamp-trained": Refine("gmvae", "relu", 24, 5, 4, (16,), 5, 4, "trained", seed=2, kind="clamp"),
    "clamp-diverging": Refine("gmvae", "tanh", 24, 5, 4, (16,), 5, 4, "diverging", seed=3, kind="clamp"),
    # ---- finite in fp32, the square is not (seed 1: at seed 0 the jitter left out 1 of 5)
    "seam": Refine("vae_gmp", "tanh", 24, 5, 3, (12, 20), 5, 4, "trained", seed=1, kind="seam"),
}


# The seam: the prior's sigma of dimension SEAM_DIM is 2e-9 and example SEAM_EXAMPLE starts SEAM_DISTANCE past the outermost
# component's mean in that dimension, so that d m of that one element is SEAM_DISTANCE / sigma^2 = 5e19: finite in fp32 and in
# fp64, its square (2.5e39) in fp64 only.
SEAM_DIM, SEAM_EXAMPLE, SEAM_SIGMA, SEAM_DISTANCE = 0, 1, 2e-9, 200.0
SEAM_BAND = (2e19, 1e20)


def refine_rule(c):
    return c.rule or ("sqrt_v" if c.regime == "trained" and c.kind in ("parity", "own_count") else "clearance")


def clamp_dims(c):
    """(the dimension that starts at sigma_0 = 2e-9, the one that starts at 200).  The first is where the prior's sigma is
    smallest: d s = 1 - (sigma / sigma_p)^2 eps^2 - (m - mu) sigma eps / sigma_p^2 pushes s DOWN from -20.03 only where sigma_p is
    of sigma's order (the diverging regime: the last term, 5e8 per unit distance, decides the sign per example); against a prior
    sigma of 0.1 and more d s is 1 and s leaves the edge upwards."""
    i = params(c)
    _, _, sg = A.prior_table(i["model"], i["d"], i["p"])
    lo = int(np.argmin(sg.min(axis=0)))
    return lo, (lo + 1) % c.L


def refine_start(c):
    """start [B, 2 L] fp32 = (mu_0, sigma_0): refine_ref.start_table, with the elements a clamp or seam case moves."""
    i = params(c)
    st = RF.start_table(i["model"], i["d"], i["p"], i["x"]).astype(np.float32)
    if c.kind == "clamp":                     # s_0 = -20.03 and 5.30: outside [-20, 5] on both sides
        lo, hi = clamp_dims(c)
        st[:, c.L + lo] = 2e-9
        st[:, c.L + hi] = 200.0
    if c.kind == "seam":
        _, mu, _ = A.prior_table(i["model"], i["d"], i["p"])
        st[SEAM_EXAMPLE, SEAM_DIM] = mu[:, SEAM_DIM].max() + SEAM_DISTANCE
        st[:, c.L + SEAM_DIM] = 1e-3          # (so that d s of the element, d m sigma eps, stays below the bound)
    return st


def refine_restated_noise(c):
    """oracle.noise at gmvae_refine's keys: eps [n_steps + R, B S, L]."""
    n_total = c.n_steps + ADAM["R"]
    return np.stack([O.noise(c.B * c.S, c.L, 1, 0, SEED, STEP * (n_total + 1) + t)[0] for t in range(n_total)]).astype(np.float32)


def refine_injected(c, eps):
    eps = np.array(eps, np.float32)
    for t, b in c.inject:
        eps[t, b * c.S:(b + 1) * c.S, :] = INF
    return eps


REFINE_KEYS = ("phi", "trace", "bounds")


def refine_run(c, eps, count="own"):
    """The statement on a case with the noise given (already injected): refine_ref.refine's dict plus `kept` and `well`."""
    i = params(c)
    rule = refine_rule(c)
    args = (i["model"], i["d"], i["p"], i["x"], refine_start(c), c.n_steps, c.S, ADAM["R"], ADAM["lr"], *ADAM["betas"],
            ADAM["adam_eps"], eps)
    ref = RF.refine(*args, rule=rule, count=count)
    ref["well"] = A.well_conditioned(ref, RF.refine(*args, rule=rule, count=count, jitter_seed=JITTER_SEED), REFINE_KEYS)
    ref["kept"] = ref["decided"] & (ref["well"] if rule == "clearance" else True)
    return ref


_REFINE_CPU = {}


def refine_cpu(name):
    if name not in _REFINE_CPU:
        c = REFINE[name]
        _REFINE_CPU[name] = refine_run(c, refine_injected(c, refine_restated_noise(c)))
    return _REFINE_CPU[name]

