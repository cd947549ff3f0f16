"""The sharding contract of GmvaeDims::row0 (include/gmvae_hip.h) -- test infrastructure, a plain module: the tables of
tests/test_shards_cpu.py (the tables against themselves, no device) and tests/test_shards.py (the device).

Part A, FAMILIES: one row per objective family and variant.  A batch of B = 11 rows is stepped whole at row0 = 5 and as three shards
of 1, 6 and 4 rows at row0 = 5, 6, 12, with in-kernel noise at (SEED, STEP); problem(id) gives the family's parameters, batch,
per-step inputs, the regenerated noise (oracle.noise at row_base = 5 * rows per example) and its fp64 statement.  The shapes are the
families' own smallest cases at B = 11; every family has a case with D % 4 != 0.

Part B, HIGH_ROWS: one entry per (noise site, boundary): Philox rows that straddle 2^31, 2^32 and the last row the entry point
admits (2^38 - 1: the 6-bit high field of csrc/aux.hpp noise_vals).  rows_of(e) gives the entry's global Philox rows,
truncated(rows, e) what a 32-bit (31-bit) row would give.  NOISE_SITES is the hand-kept list of every function in csrc/ that
calls noise_vals, with the entries that hold it."""
import contextlib
import dataclasses
import functools

import numpy as np

import count_ref as CR
import dreg_ref as DR
import gate_corners as GC
import lik_ref as LR
import oracle as O
import pmask_ref as PR
import post_comp_ref as PC
import realx_ref as RR
import wobj_ref as WR
import ytemp_ref as TR
import bdmc_cases as BK

# ------------------------------------------------------------------------------------------------------------- Part A
B, ROW0 = 11, 5
CUTS = ((0, 1), (1, 7), (7, 11))          # shards of 1, 6 and 4 rows: row0 = 5, 6, 12
SEED, STEP = 5, 3                         # (the per-family step helpers' seed and step)
PRE_TOL = 1e-5                            # hip_util.PRE_TOL: no hidden unit of a Part A case lies this close to a ReLU's kink
LOSS_RTOL, GRAD_RTOL = 2e-6, 2e-5         # shard sum against the whole-batch device step (tests/test_parallel.py's numbers)
CONTROL_RTOL = 1e-5                       # shards at row0 = 0 each miss the whole batch's loss by more than this

# include/gmvae_hip.h GMVAE_* (gmvae_amd/_lib.py has the same values; tests/test_shards_cpu.py compares them)
OBJ_MARGINAL_Y, OBJ_MARGINAL_Y_IW, GRAD_DREG, OBJ_WEIGHTS = 4, 8, 16, 64
Y_TEMP_DEV, Y_STRAIGHT_THROUGH, OBJ_PIXEL_MASK = 128, 256, 512

TAU = 0.5                                 # slot 0 of the temperatures (dims->temperature holds the decoy 1.0)
BETAS = WR.WEIGHTS                        # (beta_z, beta_y); lambda: floor_lambda of the case's own KL_y


@dataclasses.dataclass(frozen=True)
class Family:
    id: str
    kind: str                  # mask | lik | realx | count | weights | temp | dreg | iw: the step helper and the statement
    mname: str
    d: object                  # oracle.Dims, S included
    flags: int
    opt: str = None            # lik: grey | cb | gauss; realx: fixed | learned; count: poisson | nb; weights: marginal | None
    sigma: float = 1.0
    seed: int = 0              # of the parameters: moved until no hidden unit is numerically zero (test_shards_cpu asserts it)
    control: bool = False      # A5 runs on this case
    mild: bool = False         # realx: realx_ref's milder batch (large columns x 3, sigma >= 0.5), as its own S = 50 case takes


_VAE = dict(L=5, K=1, hidden=(24,))
_GMP = dict(L=5, K=3, hidden=(24,), sigma_min=0.5)
FAMILIES = [
    # the pixel mask, all three models; D = 99: the shard boundaries inside the [B][D] mask region fall off every multiple of 4
    Family("mask-vae", "mask", "vae", O.Dims(D=100, **_VAE), OBJ_PIXEL_MASK, seed=1, control=True),
    Family("mask-vae_gmp", "mask", "vae_gmp", O.Dims(D=100, **_GMP), OBJ_PIXEL_MASK),
    Family("mask-gumbel-d99", "mask", "gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), OBJ_PIXEL_MASK),
    Family("mask-gmvae-s3", "mask", "gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3), OBJ_PIXEL_MASK),
    # the likelihoods on grey-level bytes, fixed sigma
    Family("grey-vae", "lik", "vae", O.Dims(D=100, **_VAE), LR.FLAG["grey"], "grey"),
    Family("cb-gumbel-d99", "lik", "gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), LR.FLAG["cb"], "cb"),
    Family("gauss-gmvae-s3", "lik", "gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3), LR.FLAG["gauss"], "gauss", sigma=0.25),
    # fp32 x: a shard's x starts 4 * 99 * first bytes into the batch
    Family("f32-gmvae-d99", "realx", "gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)), RR.LIK_GAUSSIAN | RR.X_F32, "fixed", sigma=0.25,
           control=True),
    Family("f32-gmvae-d99-learned", "realx", "gmvae", O.Dims(D=99, L=5, K=7, hidden=(24,)),
           RR.LIK_GAUSSIAN | RR.X_F32 | RR.LIK_SCALE_LEARNED, "learned"),
    # S = 3: the milder batch.  With the x 30 columns at these dims the statement's kl is out of any fp32 evaluation's reach: the
    # same statement in torch fp32 on the CPU misses its gate 2 times over (1 to 10 times over the batch seeds 5 .. 11; the
    # device's whole-batch step missed it 1.3 times; profiles/shard_notes.md).  tests/test_shards_cpu.py holds every float case's
    # fp32 evaluation on the CPU to a quarter of the standing gates.
    Family("f32-gmvae-s3-learned", "realx", "gmvae", O.Dims(D=96, L=4, K=6, hidden=(16,), S=3),
           RR.LIK_GAUSSIAN | RR.X_F32 | RR.LIK_SCALE_LEARNED, "learned", mild=True),
    # counts (tests/count_ref.py's shapes: L = 8, hidden 64)
    Family("poisson-vae-d13-s3", "count", "vae", O.Dims(D=13, L=8, K=1, hidden=(64,), S=3), CR.FLAG["poisson"], "poisson"),
    Family("nb-vae-d13-s3", "count", "vae", O.Dims(D=13, L=8, K=1, hidden=(64,), S=3), CR.FLAG["nb"], "nb"),
    Family("nb-gmvae-d100-s3", "count", "gmvae", O.Dims(D=100, L=8, K=3, hidden=(64,), S=3), CR.FLAG["nb"], "nb", seed=1),
    # the weighted objective with its free-bits floor
    Family("weights-gumbel-d99", "weights", "gmvae", O.Dims(D=99, L=5, K=7, hidden=(24, 24), temperature=0.7), OBJ_WEIGHTS),
    Family("weights-marginal", "weights", "gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24)), OBJ_WEIGHTS | OBJ_MARGINAL_Y, "marginal",
           seed=5),
    # the device temperature, straight-through y
    Family("temp-k7-s3", "temp", "gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24), S=3), Y_TEMP_DEV),
    Family("temp-st-d99-s3", "temp", "gmvae", O.Dims(D=99, L=5, K=7, hidden=(24, 24), S=3), Y_TEMP_DEV | Y_STRAIGHT_THROUGH),
    # DReG
    Family("dreg-vae-s3", "dreg", "vae", O.Dims(D=97, L=5, K=1, hidden=(16,), S=3), GRAD_DREG),
    Family("dreg-vae_gmp-s3", "dreg", "vae_gmp", O.Dims(D=96, L=8, K=7, hidden=(16,), S=3), GRAD_DREG),
    Family("dreg-gmvae-marginal_iw-s3", "dreg", "gmvae", O.Dims(D=96, L=6, K=6, hidden=(16,), S=3), GRAD_DREG | OBJ_MARGINAL_Y_IW),
    # the importance-weighted Gumbel step without any bit
    Family("iw-gumbel-s3", "iw", "gmvae", O.Dims(D=99, L=5, K=3, hidden=(24,), S=3), 0),
]
BY_ID = {f.id: f for f in FAMILIES}
assert len(BY_ID) == len(FAMILIES)


def rows_per_example(f):
    """Philox rows per example: S, S K with y summed out."""
    return f.d.S * (f.d.K if f.flags & (OBJ_MARGINAL_Y | OBJ_MARGINAL_Y_IW) else 1)


def floor_lambda(kl_y, min_gap=1e-3):
    """The lambda of the weighted cases: the midpoint of the widest gap between two neighbouring sorted KL_y for which the floor
    (KL_y < lambda) is active for some examples on both sides of every cut and inactive for others on every side of more than
    one row."""
    v = np.sort(np.asarray(kl_y, np.float64))
    best = None
    for i in np.argsort(-np.diff(v)):
        lam = 0.5 * (v[i] + v[i + 1])
        if v[i + 1] - v[i] > min_gap and floor_split_ok(kl_y, lam):
            best = lam
            break
    assert best is not None, "no lambda splits the floor on both sides of every cut"
    return best


def floor_split_ok(kl_y, lam):
    act = np.asarray(kl_y) < lam
    for _, cut in CUTS[:-1]:
        for side in (act[:cut], act[cut:]):
            if not side.any() or (side.size > 1 and side.all()):
                return False
    return True


@dataclasses.dataclass
class Problem:
    f: Family
    model: int
    d: object
    flat: np.ndarray           # fp32, rho appended where the family learns one
    p32: dict
    x: np.ndarray              # as the device takes it: uint8 or float32 [B, D]
    eps: np.ndarray            # the regenerated noise of the whole batch at row0 = ROW0
    u: np.ndarray
    extra: dict                # mask, rho, weights, tau, t: what the statement and the per-step inputs need

    def inputs(self, a=0, b=B):
        """write_inputs' mapping for rows a .. b - 1: per-example regions are the shard's own rows."""
        f, e = self.f, self.extra
        if f.kind == "mask":
            return {"pixel_mask": e["mask"][a:b]}
        if f.kind == "lik" and f.opt == "gauss":
            return {"lik_sigma": np.array([f.sigma], np.float32)}
        if f.kind == "weights":
            return {"obj_weights": list(e["weights"]) + [0.0]}
        if f.kind == "temp":
            return {"y_temperature": [TAU]}
        return None

    def statement(self, relu_masks=None):
        """(C, g) of the family's fp64 statement on the whole batch and the regenerated noise."""
        f, e, a = self.f, self.extra, (self.model, self.d, self.p32)
        if f.kind == "mask":
            return PR.loss_and_grads(*a, self.x, self.eps, self.u, e["mask"], relu_masks=relu_masks)
        if f.kind == "lik":
            return LR.loss_and_grads(*a, self.x, self.eps, self.u, f.opt, f.sigma, relu_masks=relu_masks)
        if f.kind == "realx":
            return RR.loss_and_grads(*a, e["t"], self.eps, self.u, sigma=f.sigma, rho=e["rho"], relu_masks=relu_masks)
        if f.kind == "count":
            return CR.loss_and_grads(*a, self.x, self.eps, self.u, f.opt, e["rho"], relu_masks=relu_masks)
        if f.kind == "weights":
            return WR.loss_and_grads(*a, self.x, self.eps, self.u, e["weights"], f.opt == "marginal", relu_masks=relu_masks)
        if f.kind == "temp":
            return TR.loss_and_grads(self.d, self.p32, self.x, self.eps, self.u, TAU,
                                     straight_through=bool(f.flags & Y_STRAIGHT_THROUGH), relu_masks=relu_masks)
        if f.kind == "dreg":
            return DR.loss_and_grads(*a, self.x, self.eps, self.d.S, relu_masks=relu_masks)
        return O.loss_and_grads(*a, self.x, self.eps, self.u, np.float64, relu_masks=relu_masks)


@functools.lru_cache(maxsize=None)
def problem(id):
    f = BY_ID[id]
    model, d = O.MODEL_NAMES[f.mname], f.d
    p = O.init_params(model, d, np.random.default_rng(f.seed))
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    per = rows_per_example(f)
    eps, u = O.noise(B * per, d.L, d.K, ROW0 * per, SEED, STEP)
    u = u if model == O.MODEL_GMVAE and per == d.S else None
    x, _, _ = O.make_inputs(d, B, model)
    extra = {"rho": None}
    if f.kind == "mask":
        extra["mask"] = PR.make_mask(B, d.D)
        x = PR.flip_missing(x, extra["mask"])
    elif f.kind == "lik":
        x = LR.grey_batch(B, d.D)
    elif f.kind == "realx":
        x, rho32 = RR.real_batch(B, d.D, big=3.0, sigma_lo=0.5) if f.mild else RR.real_batch(B, d.D)
        extra["t"] = x.astype(np.float64)
        if f.opt == "learned":
            flat, extra["rho"] = CR.with_rho(flat, rho32, d.D), rho32.astype(np.float64)
    elif f.kind == "count":
        x, rho32 = CR.count_batch(B, d.D)
        if f.opt == "nb":
            flat, extra["rho"] = CR.with_rho(flat, rho32, d.D), rho32.astype(np.float64)
    P = Problem(f, model, d, flat, p32, x, eps, u, extra)
    if f.kind == "weights":
        extra["weights"] = (1.0, 1.0, 0.0)
        extra["kl_y"] = P.statement()[0]["kl_y"]
        extra["weights"] = BETAS + (floor_lambda(extra["kl_y"]),)
    return P


@functools.lru_cache(maxsize=None)
def statement(id):
    """The fp64 statement of a case: computed once, shared, left unchanged."""
    return problem(id).statement()


def min_pre_ratio(C):
    """The smallest |pre-activation| / sum |a||w| over every hidden unit of the statement.  A unit with sum |a||w| == 0 -- the
    first layer on a row that observes no pixel, under zero biases -- is 0 exactly in every arithmetic and is left out (its
    pre-activation is asserted to be 0)."""
    out = []
    for net in C["pre"].values():
        for pre, mag in net:
            live = mag > 0
            assert (pre[~live] == 0).all()
            out.append(float((np.abs(pre[live]) / mag[live]).min()))
    return min(out)


def rho_name(f):
    return {"realx": RR.LOG_SIGMA, "count": CR.LOG_DISPERSION}.get(f.kind) if f.opt in ("learned", "nb") else None


def count_entries(f):
    """The tail entries that are counts (each family's header comment in include/gmvae_hip.h): they add exactly."""
    return {"mask": (4, 6, 7), "lik": (4, 6, 7), "realx": (4, 6, 7), "count": (4, 6, 7), "weights": (4, 7)}.get(f.kind, (4,))


# ------------------------------------------------------------------------------------------------------------- Part B
TWO31, TWO32, TWO38 = 1 << 31, 1 << 32, 1 << 38
BOUNDARIES = {"2^31": TWO31, "2^32": TWO32, "last": TWO38}


def row0_for(boundary, per, nB, inside):
    """The row0 at which Philox row `boundary` falls inside example `inside` of a call of nB examples at `per` rows each (the
    example's rows straddle it where per > 1); boundary 2^38: the last row0 the entry point admits, (row0 + nB) per < 2^38."""
    if boundary == TWO38:
        return (TWO38 - 1) // per - nB
    return -(-boundary // per) - 1 - inside if per > 1 else boundary - inside


@dataclasses.dataclass(frozen=True)
class HighRow:
    id: str
    site: str                  # step | iw_bound | iw_bound_enum_y | posterior_y | posterior_component | impute | ais | ais_reverse | refine | simulate |
                               # aggregate_posterior
    boundary: str              # key of BOUNDARIES
    case: str                  # the site's own case: a gate_corners id (step), a shape of the evaluator's test file
    B: int
    per: int                   # Philox rows per example
    row0: int
    seed: int = 11
    step: int = 3
    flags: int = 0
    S: int = 1
    n: int = 0                 # evaluators: samples; chunk = 3
    env: tuple = ()


def rows_of(e):
    """The global Philox rows of the entry's call, [B * per]."""
    return [(e.row0 + b) * e.per + j for b in range(e.B) for j in range(e.per)]


def truncated(rows, e):
    """The rows a 32-bit row would give (31-bit for the 2^31 entries)."""
    m = TWO31 if e.boundary == "2^31" else TWO32
    return [r % m for r in rows]


_NOISE = O.noise


def noise_at(rows, L, K, seed, step):
    """oracle.noise of an arbitrary list of rows: (eps [n, L], u [n, K])."""
    rows = list(rows)
    out, i = [], 0
    while i < len(rows):                       # contiguous runs
        j = i
        while j + 1 < len(rows) and rows[j + 1] == rows[j] + 1:
            j += 1
        out.append(_NOISE(j - i + 1, L, K, rows[i], seed, step))
        i = j + 1
    return np.concatenate([e for e, _ in out]), np.concatenate([u for _, u in out])


@contextlib.contextmanager
def rows_truncated(e, on=True):
    """Inside: oracle.noise draws row (row mod 2^32) -- mod 2^31 for a 2^31 entry -- where it is asked for `row`: what a kernel
    that formed its Philox row in 32 bits would draw.  It swaps the attribute oracle.noise, so it reaches only code that calls
    the noise as `O.noise(...)` at call time -- every *_ref.py does (oracle/__init__.py says so beside the export).  A reference
    that bound the function at import would draw the true rows and its entry would fail the separation check (margin 0)."""
    if not on:
        yield
        return

    def patched(rows, L, K, row_base, seed, step):
        return noise_at(truncated([row_base + i for i in range(rows)], e), L, K, seed, step)
    O.noise = patched
    try:
        yield
    finally:
        O.noise = _NOISE


# the step: one corner per leading schedule word of gate_corners.CORNERS, the general schedule at S = 3 and with y summed out
STEP_CORNERS = ("mega-gmvae-D16", "mega-vae-D16", "mega-vae_gmp-D16", "fused-L8", "skinny-gmvae-D16", "skinny-vae-D16",
                "mega-gmvae-L128-K17")
GENERAL_S3 = O.Dims(D=100, L=5, K=3, hidden=(24,), S=3)          # "general-s3", "general-marginal_iw-s3" (Part A's smallest dims)
STEP_DIMS = {"general-s3": ("gmvae", GENERAL_S3, 0), "general-marginal_iw-s3": ("gmvae", GENERAL_S3, OBJ_MARGINAL_Y_IW)}
STEP_B = 8                                                       # (B <= 24: the corners' own batch; 8 for the S = 3 cases)

# the train graphs (mega2_body, mega2v_body, the first layer inside mega_fwd_bwd): the smallest `train` corner of each schedule in
# gate_corners whose batch can straddle 2^32 at row0 = rank B, rank = floor(2^32 / B) -- a batch of one row cannot
TRAIN_CORNERS = ("train-gmvae-B1023", "train-vae-panels36", "train-gmvae-D896")


def train_entry(cid):
    """The first step of a train corner's trajectory as a step entry: rows rank B .. rank B + B - 1."""
    c = GC.BY_ID[cid]
    return HighRow(cid, "step", "2^32", cid, c.B, 1, TWO32 // c.B * c.B, seed=4, step=0)


# the chunked evaluators: n = 7 in chunks of 3, the smallest dims of the respective test file
EVAL_SHAPES = {
    "iw_bound": ("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24))),                       # test_iw_bound gmvae_small: general
    "iw_bound-evalf": ("gmvae", O.Dims(D=784, L=64, K=10, hidden=(64,))),                  # ... gmvae_evalf: the fused forward
    "iw_bound-evalf-vae": ("vae", O.Dims(D=784, L=2, K=1, hidden=(64,))),                  # ... vae_evalf: evalf_rows_v
    "iw_bound_enum_y": ("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24))),
    "posterior_y": ("gmvae", O.Dims(D=100, L=5, K=7, hidden=(24, 24))),
    "posterior_component": ("vae_gmp", O.Dims(D=60, L=3, K=4, hidden=(16,))),
}
EVAL_N, EVAL_CHUNK, EVAL_B = 7, 3, 5
EVAL_SEEDS = {"iw_bound-evalf-vae": 12}      # (L = 2: at seed 11 the 2^31 entry's truncated reference sat 5 gates off, not 10)
# the chains (gmvae_ais, gmvae_ais_reverse: Philox row (row0 + b) n_chains + c) and gmvae_simulate (row0 + b): the first parity
# case of tests/bdmc_cases.py at 2 chains and 4 temperatures
CHAIN_CASE = BK.CASES[0]
CHAIN_B, CHAIN_C, CHAIN_T, CHAIN_LEAP = 4, 2, 4, 3
REFINE_S, REFINE_STEPS, REFINE_ROUNDS = 2, 3, 1      # gmvae_refine: Philox row (row0 + b) S + s, n_steps + n_eval_rounds draws
NOISE_ATOL = 2e-5                            # gmvae_noise_fill's normals against oracle.noise (tests/test_hip_parity.py)
AGG_M, AGG_N = 7, 48                         # tests/test_aggpost.py: its "gmvae" model, 48 examples, its 7-query subset
AGG_QUERIES = np.array([5, 0, 47, 5, 20, 33, 1], np.int64)
IMPUTE_CASE = "gumbel"                       # tests/impute_cases.py: B = 8, n = 7 in chunks of 3, its own seed and step


def _high_rows():
    out = []
    for bname, bnd in BOUNDARIES.items():
        for cid in STEP_CORNERS:
            c = GC.BY_ID[cid]
            out.append(HighRow(f"step-{cid}-{bname}", "step", bname, cid, c.B, 1, row0_for(bnd, 1, c.B, c.B // 2), env=c.env))
        for cid, (_, d, fl) in STEP_DIMS.items():
            per = d.S * (d.K if fl else 1)
            out.append(HighRow(f"step-{cid}-{bname}", "step", bname, cid, STEP_B, per, row0_for(bnd, per, STEP_B, 3), flags=fl, S=d.S))
        for kind, (mname, d) in EVAL_SHAPES.items():
            site = kind.split("-")[0]
            per = EVAL_N * (d.K if site in ("iw_bound_enum_y", "posterior_y") else 1)
            out.append(HighRow(f"{kind}-{bname}", site, bname, kind, EVAL_B, per, row0_for(bnd, per, EVAL_B, 2), n=EVAL_N,
                               seed=EVAL_SEEDS.get(kind, 11),
                               env=(("GMVAE_NO_EVALF", "1"),) if kind == "iw_bound" else ()))
        out.append(HighRow(f"impute-{bname}", "impute", bname, IMPUTE_CASE, 8, EVAL_N, row0_for(bnd, EVAL_N, 8, 3), seed=5, n=EVAL_N))
        for site, step in (("ais", BK.STEP), ("ais_reverse", BK.STEP_REV)):
            out.append(HighRow(f"{site}-{bname}", site, bname, "chain", CHAIN_B, CHAIN_C, row0_for(bnd, CHAIN_C, CHAIN_B, 1),
                               seed=BK.SEED, step=step))
        out.append(HighRow(f"refine-{bname}", "refine", bname, "chain", CHAIN_B, REFINE_S, row0_for(bnd, REFINE_S, CHAIN_B, 1),
                           seed=BK.SEED, step=BK.STEP))
        # Engine.aggregate_posterior: M = 7 queries, row row0 + m; the 2^32 entry at a multiple of M, the default row0 of a rank
        r0 = TWO32 // AGG_M * AGG_M if bname == "2^32" else row0_for(bnd, 1, AGG_M, 3)
        out.append(HighRow(f"aggregate_posterior-{bname}", "aggregate_posterior", bname, "gmvae", AGG_M, 1, r0))
        out.append(HighRow(f"simulate-{bname}", "simulate", bname, "chain", 8, 1, row0_for(bnd, 1, 8, 3), seed=BK.SEED, step=BK.STEP))
    return out


HIGH_ROWS = _high_rows()
HIGH_BY_ID = {e.id: e for e in HIGH_ROWS}
assert len(HIGH_BY_ID) == len(HIGH_ROWS)

# every function in gmvae_amd/csrc that calls noise_vals: (file, function, the HIGH_ROWS sites that run it past 2^32 -- empty: the
# site is listed, its rows are not yet held above a few thousand by any device test)
NOISE_SITES = [
    ("aux.hpp", "noise_item", ("step-general-s3", "step-general-marginal_iw-s3", "step-mega-gmvae-L128-K17",
                               "aggregate_posterior")),                                                        # gmvae_noise_fill
    ("iwbound.hpp", "iw_noise_fill", ("iw_bound", "iw_bound_enum_y", "posterior_y", "posterior_component")),
    ("evalf.hpp", "evalf_rows", ("iw_bound-evalf",)),
    ("evalf.hpp", "evalf_rows_v", ("iw_bound-evalf-vae",)),
    ("mega.hpp", "mega_fwd_bwd", ("step-mega-gmvae-D16", "step-mega-vae-D16", "step-mega-vae_gmp-D16")),
    ("skinny.hpp", "sk_gemm", ("step-skinny-vae-D16",)),
    ("skinny.hpp", "sk_ypath", ("step-skinny-gmvae-D16",)),
    ("skinny.hpp", "sk_ypath_r", ()),              # more than 768 batch rows: past the sizes of this table
    ("mega2.hpp", "mega2_body", ("train-gmvae-B1023",)),           # the train graphs' schedules (step_dev): TRAIN_CORNERS
    ("mega2v.hpp", "mega2v_body", ("train-vae-panels36",)),
    ("ais.hpp", "ais_noise", ("ais", "ais_reverse", "refine")),
    ("bdmc.hpp", "sim_rows", ("simulate",)),
    ("impute.hip", "impute_merge", ("impute",)),
]
NOT_HELD = {("skinny.hpp", "sk_ypath_r")}          # the rows of NOISE_SITES that no entry runs: tests/test_shards_cpu.py holds the two together


# ---- the references of Part B: the statement of the site's own test file on oracle.noise at the entry's rows; wrong=True: at the
# rows a 32-bit truncation would give.  margin_*: the worst error of `got` against `ref` as a fraction of the gate the device
# test applies (<= 1 passes); tests/test_shards_cpu.py asserts margin(reference at the truncated rows) > 10.
SEPARATION = 10.0


def step_setup(e):
    """(model, Dims with S, flat fp32, p32, x) of a step entry."""
    if e.case in STEP_DIMS:
        mname, d, _ = STEP_DIMS[e.case]
    else:
        c = GC.BY_ID[e.case]
        mname, d = c.model, c.d
    model = O.MODEL_NAMES[mname]
    flat = O.pack(model, d, O.init_params(model, d, np.random.default_rng(e.B)), np.float32)
    x, _, _ = O.make_inputs(d, e.B, model)
    return model, d, flat, O.unpack(model, d, flat.astype(np.float64)), x


def step_reference(e, wrong=False, relu_masks=None):
    """(C, g) of compare_step's statement (tests/ymarg_iw_ref.py with y summed out) on the regenerated noise."""
    import ymarg_iw_ref as YI
    model, d, flat, p32, x = step_setup(e)
    with rows_truncated(e, wrong):
        eps, u = O.noise(e.B * e.per, d.L, d.K, e.row0 * e.per, e.seed, e.step)
    if e.flags & OBJ_MARGINAL_Y_IW:
        return YI.loss_and_grads(d, p32, x, eps, d.S, relu_masks=relu_masks)
    return O.loss_and_grads(model, d, p32, x, eps, u if model == O.MODEL_GMVAE else None, np.float64, relu_masks=relu_masks)


def margin_step(e, got, ref, rtol=1e-4):
    """got, ref: (C-like dict of batch means loss / nll / kl / nent, {name: gradient}): hip_util.tail_gates' and check_grads'
    gates."""
    (Ca, ga), (Cb, gb) = got, ref
    m = [abs(Ca["loss"] - Cb["loss"]) / (rtol * abs(Cb["loss"])), abs(Ca["nll"] - Cb["nll"]) / (rtol * abs(Cb["nll"])),
         abs(Ca["kl"] - Cb["kl"]) / (rtol * max(abs(Cb["kl"]), 1.0)), abs(Ca["nent"] - Cb["nent"]) / (rtol * max(abs(Cb["nent"]), 1.0))]
    m += [np.abs(ga[k] - gb[k]).max() / (rtol * max(np.abs(gb[k]).max(), 1e-6)) for k in gb]
    return float(max(m))


def eval_setup(e):
    """(model, Dims, flat fp32, x) of an evaluator entry: the _setup of the evaluator's own test file (non-zero biases, a
    non-uniform pi for the VAE_GMP)."""
    mname, d = EVAL_SHAPES[e.case]
    model = O.MODEL_NAMES[mname]
    p = O.init_params(model, d, np.random.default_rng(0))
    if e.site != "iw_bound":
        for k in p:
            if k.endswith("/b"):
                p[k] = np.random.default_rng(7).normal(0, 0.3, p[k].shape)
    if e.site == "posterior_component":
        p["mixture_logits"] = np.random.default_rng(9).normal(0, 1.0, p["mixture_logits"].shape)
    flat = O.pack(model, d, p, np.float32)
    x, _, _ = O.make_inputs(d, e.B, model, seed_x=100)
    return model, d, flat, x


def _lse(v, axis=None):
    return PC.lse(v, axis)


def ess_of(lw):
    lw = np.asarray(lw, np.float64).ravel()
    return float(np.exp(2.0 * _lse(lw) - _lse(2.0 * lw)))


def eval_reference(e, wrong=False):
    """The outputs of the evaluator in fp64, as its own test file states them, and lw = the log weights behind them."""
    import ymarg_ref as YM
    model, d, flat, x = eval_setup(e)
    p64 = O.unpack(model, d, flat.astype(np.float64))
    n = e.n
    with rows_truncated(e, wrong):
        if e.site == "iw_bound":                     # tests/test_iw_bound.py oracle_bound
            out = []
            for b in range(e.B):
                eps, u = O.noise(n, d.L, d.K, (e.row0 + b) * n, e.seed, e.step)
                Cb = O.forward(model, dataclasses.replace(d, S=n), p64, x[b:b + 1], eps, u if model == O.MODEL_GMVAE else None)
                out.append(Cb["bound"][0])
            return {"bound": np.array(out)}
        if e.site == "posterior_component":          # tests/post_comp_ref.py
            lw = PC.log_w(d, flat, x, n, e.row0, e.seed, e.step)
            return dict(PC.statement(lw), lw=lw)
        lw, ml = [], []                              # tests/test_iw_enum.py fp64_bound, tests/test_posterior_y.py fp64_log_w
        for b in range(e.B):
            eps = O.noise(n * d.K, d.L, d.K, (e.row0 + b) * n * d.K, e.seed, e.step)[0]
            Cb, _ = YM.loss_and_grads(d, p64, np.repeat(x[b:b + 1], n, 0), eps)
            lw.append(Cb["rows"][:, 3].reshape(n, d.K))
            ml.append(-Cb["loss"])
    lw = np.array(lw)
    if e.site == "iw_bound_enum_y":
        return {"bound": np.array([_lse(lw[b]) - np.log(n) for b in range(e.B)]), "mean_logw": np.array(ml), "lw": lw}
    lj = _lse(lw, axis=1) - np.log(n)
    return {"log_joint": lj, "log_post": PC.log_softmax(lj), "ess": np.array([ess_of(lw[b]) for b in range(e.B)]), "lw": lw}


def margin_eval(e, got, ref):
    """got: the device's outputs (hip_util.chunked_call's dict) or another reference; ref: eval_reference's.  The standing gates of
    the site's own test file."""
    f = lambda k: np.asarray(got[k], np.float64)
    if e.site in ("iw_bound", "iw_bound_enum_y"):
        m = [np.max(np.abs(f("bound") - ref["bound"]) / (1e-4 * np.abs(ref["bound"])))]
        if e.site == "iw_bound_enum_y":
            m.append(np.max(np.abs(f("mean_logw") - ref["mean_logw"]) / (1e-4 * np.abs(ref["mean_logw"]))))
        return float(max(m))
    ess = f("stats")[:, 3] if "stats" in got else f("ess")
    delta = 1e-4 * np.abs(ref["lw"]).reshape(e.B, -1).max(1)
    lj = ref["log_joint"]
    return float(max(np.max(np.abs(f("log_joint") - lj) / (1e-4 * np.abs(lj))),
                     np.max(np.abs(f("log_post") - ref["log_post"]) / (2e-4 * np.abs(lj).max(1, keepdims=True))),
                     np.max(np.abs(np.log(ess / ref["ess"])) / (4 * delta))))


def impute_reference(e, wrong=False):
    """(samples, estimate) of tests/impute_ref.py at the entry's rows."""
    import impute_cases as IC
    import impute_ref as IR
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(e.case)
    with rows_truncated(e, wrong):
        s = IR.samples(model, d, p32, xf, m, e.n, IC.M_DRAWS, e.seed, e.step, e.row0)
    return s, IR.estimate(s["lw"], s["lam"], s["hid"], s["g"], s["z"])


def margin_impute(logw, ref_lw):
    """The log weights at tests/test_impute.py's row gate."""
    return float(np.max(np.abs(np.asarray(logw, np.float64) - ref_lw) / (1e-4 * np.maximum(np.abs(ref_lw), 1.0))))


def chain_dims():
    """(model, Dims) of the chain sites' case."""
    return BK.unpack_case(CHAIN_CASE)[:2]


def chain_noise(e, wrong=False):
    """The draws of a chain site restated on the CPU (tests/bdmc_cases.py): (eps, u) of the chains, (eps, u, ux) of
    gmvae_simulate."""
    _, d = chain_dims()
    with rows_truncated(e, wrong):
        if e.site == "simulate":
            return BK.cpu_sim_noise(e.B, d, e.row0, e.seed, e.step)
        if e.site == "refine":                   # tests/test_refine.py device_noise: step (n_total + 1) + t, t < n_total
            nt = REFINE_STEPS + REFINE_ROUNDS
            return (np.stack([O.noise(e.B * REFINE_S, d.L, 1, e.row0 * REFINE_S, e.seed, e.step * (nt + 1) + t)[0] for t in range(nt)]),)
        return BK.cpu_chain_noise(CHAIN_T, e.B * CHAIN_C, d.L, e.row0 * CHAIN_C, e.seed, e.step)


def margin_noise(got, ref):
    """The normals at NOISE_ATOL (the uniforms, which the device test holds bit for bit, at the same scale)."""
    return float(max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / NOISE_ATOL for a, b in zip(got, ref)))


# ---- gmvae_binarize: the Philox counter holds the quad's position in the GLOBAL batch, out_row0 * (D / 4) + q (csrc/aux.hpp), in 62
# bits.  D = 16, 8 rows: (name, out_row0) with the quad index crossing 2^31 and 2^32 inside the batch and ending at 2^62 - 1
BIN_B, BIN_D = 8, 16
BINARIZE = (("2^31", TWO31 // 4 - 3), ("2^32", TWO32 // 4 - 3), ("last", (1 << 62) // 4 - BIN_B))


def binarize_case(out_row0, wrong=0, seed=11, step=3):
    """(pixels uint8 [8, 16], the reference's x [8, 16]); wrong = 2^32 or 2^31: the uniforms of a quad index taken modulo it."""
    pix = np.random.default_rng(3).integers(0, 256, (BIN_B, BIN_D), dtype=np.uint8)
    if not wrong:
        return pix, O.binarize(pix, np.arange(BIN_B), seed, step, out_row0)
    rows = [O.binarize(pix, np.array([b]), seed, step, 0)[0] * 0 for b in range(BIN_B)]
    qpr = BIN_D // 4
    for b in range(BIN_B):
        for j in range(qpr):                     # one quad at a time at its truncated position (out_row0 = q / qpr rows of one quad)
            q = ((out_row0 + b) * qpr + j) % wrong
            rows[b][4 * j:4 * j + 4] = O.binarize(pix[b:b + 1, 4 * j:4 * j + 4], np.array([0]), seed, step, q)[0]
    return pix, np.stack(rows)


def aggpost_case():
    """(model name, Dims, model id, fp32-exact parameters, flat fp32, x uint8 [48, D]): tests/test_aggpost.py make_engine's "gmvae"
    model (non-zero biases), without the engine."""
    mname, d = "gmvae", O.Dims(D=64, L=8, K=5, hidden=(32,))
    model = O.MODEL_NAMES[mname]
    p = O.init_params(model, d, np.random.default_rng(5))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(6).normal(0, 0.3, p[k].shape)
    flat = O.pack(model, d, p, np.float32)
    x = (np.random.default_rng(7).random((AGG_N, d.D)) < 0.5).astype(np.uint8)
    return mname, d, model, O.unpack(model, d, flat), flat, x


def aggpost_reference(e, wrong=False):
    """(z [M, L], k [M]) of tests/aggpost_ref.py's sample at the entry's rows."""
    import aggpost_ref as AG
    mname, d, model, p, flat, x = aggpost_case()
    comps = AG.components(model, d, p, x)
    with rows_truncated(e, wrong):
        return AG.sample(model, d, comps, AGG_QUERIES, e.row0, e.seed, e.step)


def margin_aggpost(z, z_ref):
    """tests/test_aggpost.py gate_err at its 1e-4: |z - ref| / max(1, |ref|)."""
    z_ref = np.asarray(z_ref, np.float64)
    return float(np.max(np.abs(np.asarray(z, np.float64) - z_ref) / np.maximum(1.0, np.abs(z_ref))) / 1e-4)
