"""The cases of tests/test_objectives_saturated*.py: the objective variants' training steps (y summed out, importance-weighted,
observed labels, the weighted objective, DReG) OUTSIDE the Xavier regime -- test infrastructure, a plain module.

Parameters are test_saturated.saturate's, in two regimes:
    trained    q-head raw sigma over [-8, 8], the prior head's over [-2, 2], largest |lambda| 60: nll and kl of the same order,
               so both sides of encoder_gmm's gradient are visible to a gate that is relative to the tensor's maximum
    diverging  both heads over [-20, 20] (sigma from 2e-9 to 20): the loss is the KL term alone, 1e6 and more
with encoder_y's logits scaled by `logit` (15: nent of a few thousandths; 40: q(y|x) one-hot, its smallest entries zero in fp32).
They go through oracle.pack(..., float32) and oracle.unpack, so the statement sees what the device sees.  The fp64 statement of
a case is computed once (statement()) and shared by every test that needs it; nothing modifies it."""
import dataclasses
import math

import numpy as np

import dreg_ref as DR
import oracle as O
import semisup_ref as SR
import wobj_ref as WR
import ymarg_ref as YM
from test_saturated import U_MAX, saturate

REGIMES = {"trained": dict(span=8.0, prior_span=2.0, lam=60.0), "diverging": dict(span=20.0, prior_span=20.0, lam=60.0)}
ALPHA = 0.7                     # the classification weight of the labelled cases (tests/test_semisup.py's)
WEIGHTS = WR.WEIGHTS            # (beta_z, beta_y) of the weighted cases (tests/test_wobj.py's)

H24X2 = O.Dims(D=100, L=5, K=7, hidden=(24, 24))
ONE_LAUNCH = O.Dims(D=784, L=64, K=10, hidden=(64,))
S3 = O.Dims(D=200, L=8, K=10, hidden=(64,))
K80 = O.Dims(D=64, L=4, K=80, hidden=(16,))
S65 = O.Dims(D=100, L=5, K=3, hidden=(24,))
VAE = O.Dims(D=96, L=5, K=1, hidden=(16,))
GMP = O.Dims(D=96, L=8, K=7, hidden=(16,))
K1 = O.Dims(D=100, L=5, K=1, hidden=(24,))


@dataclasses.dataclass(frozen=True)
class Case:
    path: str                   # marginal | marginal_iw | labels | dreg | weights: the statement and the driver
    mname: str
    d: object                   # oracle.Dims (S left at 1: the sample count is the field below)
    B: int
    S: int = 1
    regime: str = "trained"
    logit: float = 15.0
    seed: int = 0
    dreg: bool = False          # GMVAE_GRAD_DREG on top of the path
    labels: str = None          # pattern (test_semisup._labels') | argmax | argmin of the statement's q
    gumbel: bool = False        # weights: one Gumbel draw of y instead of the sum over k
    lam: str = None             # weights: split (wobj_ref.split_lambda) | all_floor (ln K + 0.5) | none (0)


def _c(path, mname, d, B, **kw):
    return Case(path, mname, d, B, **kw)


CASES = {
    # ---- y summed out, S = 1: ymarg_rows
    "marginal-trained-logit15": _c("marginal", "gmvae", H24X2, 8),
    "marginal-trained-logit40": _c("marginal", "gmvae", H24X2, 8, logit=40.0),
    "marginal-diverging-logit15": _c("marginal", "gmvae", H24X2, 8, regime="diverging"),
    "marginal-diverging-logit40": _c("marginal", "gmvae", H24X2, 8, regime="diverging", logit=40.0),
    # (logit 40, not 15: on the two-layer y encoder above the smallest q is 2e-17 even at 40; this one-layer encoder at 40 is
    # the marginal path's case with q_bk exactly 0 in fp32 -- the condition of tests/test_objectives_saturated_cpu.py)
    "marginal-one-launch-sizes": _c("marginal", "gmvae", ONE_LAUNCH, 16, logit=40.0),
    # ---- y summed out, S importance samples: ymarg_iw_rows
    "iw-s3-trained": _c("marginal_iw", "gmvae", S3, 6, S=3, logit=40.0),
    "iw-s3-diverging": _c("marginal_iw", "gmvae", S3, 6, S=3, regime="diverging", logit=40.0),
    "iw-k80-s2-trained": _c("marginal_iw", "gmvae", K80, 5, S=2),                     # the lane loop's second pass over k
    "iw-k3-s65-trained": _c("marginal_iw", "gmvae", S65, 4, S=65),                    # S > 64
    # ---- DReG: z_head_bwd_dreg
    "dreg-iw-s3-trained": _c("marginal_iw", "gmvae", S3, 6, S=3, logit=40.0, dreg=True),
    "dreg-iw-s3-diverging": _c("marginal_iw", "gmvae", S3, 6, S=3, regime="diverging", logit=40.0, dreg=True),
    "dreg-vae-trained": _c("dreg", "vae", VAE, 5, S=3, dreg=True),
    "dreg-vae-diverging": _c("dreg", "vae", VAE, 5, S=3, regime="diverging", dreg=True),
    "dreg-vae_gmp-trained": _c("dreg", "vae_gmp", GMP, 5, S=3, dreg=True),
    "dreg-vae_gmp-diverging": _c("dreg", "vae_gmp", GMP, 5, S=3, regime="diverging", dreg=True),
    # ---- observed labels: ymarg_sup_rows, sup_tail
    "labels-s1-pattern": _c("labels", "gmvae", H24X2, 8, logit=40.0, labels="pattern"),
    "labels-s1-argmax": _c("labels", "gmvae", H24X2, 8, logit=40.0, labels="argmax"),
    "labels-s1-argmin": _c("labels", "gmvae", H24X2, 8, logit=40.0, labels="argmin"),
    "labels-s1-diverging-pattern": _c("labels", "gmvae", H24X2, 8, regime="diverging", logit=40.0, labels="pattern"),
    "labels-s3-pattern": _c("labels", "gmvae", S3, 6, S=3, logit=40.0, labels="pattern"),
    "labels-s3-argmax": _c("labels", "gmvae", S3, 6, S=3, logit=40.0, labels="argmax"),
    "labels-s3-argmin": _c("labels", "gmvae", S3, 6, S=3, logit=40.0, labels="argmin"),
    "labels-s3-diverging-argmin": _c("labels", "gmvae", S3, 6, S=3, regime="diverging", logit=40.0, labels="argmin"),
    "labels-dreg-s3-pattern": _c("labels", "gmvae", S3, 6, S=3, logit=40.0, labels="pattern", dreg=True),
    "labels-dreg-s3-argmin": _c("labels", "gmvae", S3, 6, S=3, logit=40.0, labels="argmin", dreg=True),
}
# ---- the weighted objective: wobj_rows, ymarg_wobj_rows, y_head_bwd_w, wobj_tail at tests/wobj_ref.py's shapes
for _n, (_m, _marg, _d, _B) in WR.CASES.items():
    _gm = _m == "gmvae"
    CASES[f"weights-{_n}-split"] = _c("weights", _m, _d, _B, gumbel=_gm and not _marg, lam="split" if _gm else "none")
for _n in ("gumbel", "marginal"):
    _m, _marg, _d, _B = WR.CASES[_n]
    CASES[f"weights-{_n}-all-floor"] = _c("weights", _m, _d, _B, gumbel=not _marg, lam="all_floor")
    CASES[f"weights-{_n}-diverging-split"] = _c("weights", _m, _d, _B, gumbel=not _marg, lam="split", regime="diverging")
    CASES[f"weights-{_n}-diverging-all-floor"] = _c("weights", _m, _d, _B, gumbel=not _marg, lam="all_floor", regime="diverging")
    # lambda = 0 where q(y|x) is one-hot (one-layer y encoder, logit 40): no floor applies.  (The one-launch sizes, not K = 80:
    # there the smallest q at logit 40 is 2e-26, here it is 0 in fp32 -- the weighted path's case of that condition.)
    _m, _marg, _d, _B = WR.CASES[f"{_n}-one-launch-sizes"]
    CASES[f"weights-{_n}-one-launch-sizes-logit40-no-floor"] = _c("weights", _m, _d, _B, gumbel=not _marg, lam="none", logit=40.0)
    # ... and where KL(q(y|x) || uniform) is exactly 0 = lambda (K = 1: nent = -ln K bit for bit): still no floor
    CASES[f"weights-{_n}-K1-no-floor"] = _c("weights", "gmvae", K1, 8, gumbel=_n == "gumbel", lam="none")
CASES["weights-vae-diverging"] = _c("weights", "vae", WR.CASES["vae"][2], 9, lam="none", regime="diverging")
CASES["weights-vae_gmp-diverging"] = _c("weights", "vae_gmp", WR.CASES["vae_gmp"][2], 9, lam="none", regime="diverging")


# ---- the forward-only consumers of the same terms (gmvae_iw_bound_enum_y, gmvae_posterior_y, gmvae_posterior_component), on
# their own Philox noise.  (logit 120, not 40: on this two-layer y encoder the smallest q at 40 is 2e-17; the posterior must be
# finite and sum to 1 where q_bk is exactly 0 in fp32.)
FORWARD = {
    "forward-h24x2-trained": _c("forward", "gmvae", H24X2, 8, logit=120.0),
    "forward-vae_gmp-trained": _c("forward", "vae_gmp", GMP, 5),
}
FORWARD_N, FORWARD_CHUNK = 6, 3


def names(path=None, **kw):
    """The names of the cases of a path (all: None) whose fields equal kw."""
    return [n for n, c in CASES.items() if (path is None or c.path == path) and all(getattr(c, k) == v for k, v in kw.items())]


_INPUTS, _REF, _LAM, _Q = {}, {}, {}, {}


def _rows_per_x(c):
    return c.S * (c.d.K if c.mname == "gmvae" and not c.gumbel else 1)


def inputs(name):
    """dict(model, d, B, S, flat (fp32), p32 (flat in fp64, unpacked), x, eps, u) of a case.  Cases that differ in the objective
    alone (labels, DReG, lambda) share their parameters and noise: the key leaves those fields out."""
    c = CASES.get(name) or FORWARD[name]
    key = (c.mname, repr(c.d), c.B, c.S, c.regime, c.logit, c.seed, c.gumbel)
    if key not in _INPUTS:
        model = O.MODEL_NAMES[c.mname]
        rng = np.random.default_rng(1000 * c.seed + c.B + c.d.L)
        x, _, u = O.make_inputs(c.d, c.B, model, seed_x=100 + c.seed)
        p = saturate(model, c.d, O.init_params(model, c.d, rng), rng, x, logit=c.logit, **REGIMES[c.regime])
        flat = O.pack(model, c.d, p, np.float32)
        p32 = O.unpack(model, c.d, flat.astype(np.float64))
        eps = np.random.default_rng(c.seed + 1).standard_normal((c.B * _rows_per_x(c), c.d.L)).astype(np.float32)
        if c.gumbel:            # the uniform stream's two extremes, where tests/test_saturated.py::test_eager_step_saturated puts them
            if c.d.K > 1:
                u[0, 0], u[1, c.d.K - 1] = O.TINY_F32, U_MAX
            u[2, :], u[3, :] = U_MAX, O.TINY_F32
            u[c.B - 1, min(1, c.d.K - 1)] = O.TINY_F32
        else:
            u = None
        _INPUTS[key] = dict(model=model, d=c.d, B=c.B, S=c.S, flat=flat, p32=p32, x=x, eps=eps, u=u)
    return _INPUTS[key]


def q_of(name):
    """softmax(logits) [B, K] of the fp64 statement at the case's parameters (it does not depend on the objective)."""
    c = CASES.get(name) or FORWARD[name]
    i = inputs(name)
    key = id(i["flat"])
    if key not in _Q:
        logits = YM._mlp({k: YM.torch.tensor(v) for k, v in i["p32"].items()}, "encoder_y", len(c.d.hidden) + 1,
                         YM.torch.tensor(np.asarray(i["x"]), dtype=YM.torch.float64), c.d.act, None, [])
        _Q[key] = YM.torch.softmax(logits, dim=1).numpy()
    return _Q[key]


def labels_of(name):
    """The observed components [B] int32 of a case (all -1 off the labels path)."""
    c = CASES[name]
    if c.labels is None:
        return np.full(c.B, -1, np.int32)
    if c.labels == "pattern":                       # 0, K - 1, K (out of range: unlabelled) and -1 among them
        from test_semisup import _labels
        return _labels(c.d.K, c.B, c.seed)
    q = q_of(name)
    return (q.argmax(1) if c.labels == "argmax" else q.argmin(1)).astype(np.int32)


def weights_of(name):
    """(beta_z, beta_y, lambda) of a weighted case; `split`: the midpoint of the widest gap of the case's own sorted KL_y
    (wobj_ref.split_lambda asserts the gap > 1e-3 nat and examples on both sides)."""
    c = CASES[name]
    if c.lam == "all_floor":
        return WEIGHTS + (math.log(c.d.K) + 0.5,)
    if c.lam == "split":
        i = inputs(name)
        key = id(i["flat"])
        if key not in _LAM:
            C0, _ = WR.loss_and_grads(i["model"], c.d, i["p32"], i["x"], i["eps"], i["u"], (1.0, 1.0, 0.0), not c.gumbel)
            _LAM[key] = WR.split_lambda(C0["kl_y"])
        return WEIGHTS + (_LAM[key],)
    return WEIGHTS + (0.0,)


def statement(name):
    """(C, g) of the fp64 statement of the case's path -- computed once, shared, left unchanged."""
    if name not in _REF:
        c = CASES[name]
        i = inputs(name)
        model, d, p, x, eps = i["model"], c.d, i["p32"], i["x"], i["eps"]
        if c.path == "marginal":
            _REF[name] = YM.loss_and_grads(d, p, x, eps)
        elif c.path in ("marginal_iw", "labels"):
            _REF[name] = SR.loss_and_grads(d, p, x, eps, c.S, labels_of(name), ALPHA, estimator="dreg" if c.dreg else "standard")
        elif c.path == "dreg":
            _REF[name] = DR.loss_and_grads(model, d, p, x, eps, c.S)
        else:
            marginal = model == O.MODEL_GMVAE and not c.gumbel
            _REF[name] = WR.loss_and_grads(model, d, p, x, eps, i["u"], weights_of(name), marginal)
    return _REF[name]


def facts(name):
    """What tests/test_objectives_saturated_cpu.py asserts on and profiles/objectives_saturated_notes.md records: dict(loss,
    nll, kl, nent, min_q = min_bk q_bk (None: no y), max_v = the largest softmax_s weight of a sample group (None at S = 1),
    finite = every term and gradient finite, ce_max = the largest -ln q_bc of a labelled example (None: none labelled))."""
    c = CASES[name]
    C, g = statement(name)
    out = {k: C[k] for k in ("loss", "nll", "kl", "nent")}
    out["finite"] = bool(np.isfinite([C[k] for k in ("loss", "nll", "kl", "nent")]).all() and
                         all(np.isfinite(v).all() for v in g.values()))
    out["min_q"] = float(q_of(name).min()) if c.mname == "gmvae" else None
    out["max_v"] = float(np.max(C["v"])) if c.S > 1 else None
    out["ce_max"] = None
    if c.path == "labels" and C["n_labelled"]:
        lab = C["labelled"]
        lg = C["logits"][lab]                      # (log-softmax from the logits: q itself may underflow even in fp64)
        lnq = lg[np.arange(lab.sum()), labels_of(name)[lab]] - (lg.max(1) + np.log(np.exp(lg - lg.max(1, keepdims=True)).sum(1)))
        out["ce_max"] = float((-lnq).max())
    return out
