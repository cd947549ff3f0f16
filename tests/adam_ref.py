"""fp64 statement of one TF-Adam update (TF1 ApplyAdam; csrc/adam.hpp adam_update) and the per-element bounds an fp32
evaluation of it has to stay inside -- test infrastructure, a plain module: the checker of tests/test_optimizer_sites*.py.

The update is elementwise.  Given the fp32 values a device held BEFORE a step -- p, m, v -- the gradient SUM it left in the
gradient buffer, the count in tail[4] and the step t it applied, predict() gives (p', m', v') in fp64, and bounds() how far
an fp32 implementation may be from that: a few roundings, counted below.  Nothing here depends on a device's output.

    gj = g / count
    m' = m + (gj - m) (1 - b1)
    v' = v + (gj^2 - v) (1 - b2)
    alpha_t = lr sqrt(1 - b2^t) / (1 - b1^t)
    p' = p - alpha_t m' / (sqrt(v') + eps)               (eps next to the UNCORRECTED sqrt(v'): torch.optim.Adam differs)

The hyperparameters are held in fp32 the way TF holds them in T (1 - b2 = 1 - float32(0.999), oracle.adam_tf_step)."""
import numpy as np

U = 2.0 ** -24                 # fp32 unit roundoff
TINY = 2.0 ** -126             # smallest normal fp32: what one operation may lose to underflow (gradual or flushed)

# the hyperparameter sets (lr, b1, b2, eps) and the step counters t0 (the step applied is t0 + 1) of the optimizer-site tests
HP = {
    1: (1e-3, 0.9, 0.999, 1e-8),        # TF's defaults
    2: (3e-4, 0.5, 0.9, 1e-3),          # eps comparable to sqrt(v): its placement and plumbing show; every value differs from the default
    3: (1e-3, 0.0, 0.999, 1e-8),        # TF accepts b1 = 0; ln b1 = -inf in the fp32 form of alpha_t
    4: (1e-3, 0.9, 0.9999, 1e-8),
}
T0 = (0, 999, 10 ** 6, 2 ** 24)
T0_WRAP = 2 ** 32 - 2                   # with three steps the low 32 bits of t pass through 0


def _f32(x):
    return np.float64(np.float32(x))


def one_minus(b):
    """1 - b as the device and TF form it: in fp32."""
    return np.float64(np.float32(1) - np.float32(b))


def alpha_fp64(t, lr, b1, b2):
    """alpha_t from fp64 pow on the fp32 hyperparameters (adam_tf, finalize_adam, adam_tf_img, m3_alpha)."""
    lr, b1, b2, t = _f32(lr), _f32(b1), _f32(b2), np.float64(t)
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def alpha_fp32(t, lr, b1, b2):
    """alpha_t in the fp32 form of csrc/dwadam.hpp and csrc/skinny.hpp, evaluated in numpy.float32:
    lr sqrtf(-expm1f(tf ln b2)) / (-expm1f(tf ln b1)), ln b rounded from double, tf = (float)t."""
    f = np.float32
    with np.errstate(divide="ignore"):
        ln1, ln2 = f(np.log(_f32(b1))), f(np.log(_f32(b2)))
    tf = f(int(t))
    return f(lr) * np.sqrt(-np.expm1(tf * ln2, dtype=f), dtype=f) / (-np.expm1(tf * ln1, dtype=f))


def d_alpha_fp32(t, b1, b2):
    """The measured relative error of the fp32 form against the fp64 one at (t, b1, b2), doubled (lr = 1e-3: it enters both
    forms as one factor).  A CPU measurement: the allowance of the fp32-form sites in bounds()."""
    a64 = alpha_fp64(t, 1e-3, b1, b2)
    return 2.0 * abs(float(alpha_fp32(t, 1e-3, b1, b2)) - a64) / a64


D_ALPHA_FP64 = 2 * U           # the fp64 form, rounded to fp32 once


def predict(p, m, v, gsum, count, t, lr, b1, b2, eps):
    """(p', m', v', upd) in fp64 from the fp32 values the device held; upd = alpha_t m' / (sqrt(v') + eps)."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, gsum))
    gj = g / np.float64(count)
    m2 = m + (gj - m) * one_minus(b1)
    v2 = v + (gj * gj - v) * one_minus(b2)
    upd = alpha_fp64(t, lr, b1, b2) * m2 / (np.sqrt(v2) + _f32(eps))
    return p - upd, m2, v2, upd


def bounds(p, m, v, gsum, count, t, lr, b1, b2, eps, d_alpha=D_ALPHA_FP64):
    """(dm, dv, dp): how far an fp32 evaluation of the statement may be from predict(), per element, u = 2^-24:
        dm = 4u (|gj| + |m|) + 4 TINY
        dv = 4u (gj^2 + v) + 4 TINY                      (no cancellation: v' >= b2 v)
        dp = u |p'| + alpha_t (dm + |m'| dv / (2 sqrt(v') (sqrt(v') + eps))) / (sqrt(v') + eps) + |upd| (6u + d_alpha)
    The 4 and the 6 count adam_update's roundings with about a factor of two to spare -- m': g * (1 / count) (two: the
    reciprocal and the product), __fsub_rn, __fmaf_rn; v': the same gj squared, two __fmaf_rn; p': __fmul_rn, __fsqrt_rn,
    __fadd_rn, __fdiv_rn, alpha_t's own rounding is d_alpha's, and the final __fsub_rn is the u |p'| term.
    4 TINY: each of those operations may also lose up to the smallest normal number to underflow (gj^2 of a gradient below
    1e-19 is not a normal fp32 number), an absolute term a relative count cannot carry: one TINY per rounding counted.
    d_alpha: the relative error of the site's alpha_t -- D_ALPHA_FP64 for the fp64 form, d_alpha_fp32(t, b1, b2) for the fp32 one."""
    p2, m2, v2, upd = predict(p, m, v, gsum, count, t, lr, b1, b2, eps)
    m, v, g = (np.asarray(a, np.float64) for a in (m, v, gsum))
    gj = g / np.float64(count)
    dm = 4 * U * (np.abs(gj) + np.abs(m)) + 4 * TINY
    dv = 4 * U * (gj * gj + v) + 4 * TINY
    s = np.sqrt(v2)
    den = s + _f32(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s > 0, dv / (2 * s), np.sqrt(dv))          # (v' = 0: |sqrt(x) - 0| <= sqrt(dv) for |x| <= dv)
        dp = U * np.abs(p2) + alpha_fp64(t, lr, b1, b2) * (dm + np.abs(m2) * ds / den) / den + np.abs(upd) * (6 * U + d_alpha)
    return dm, dv, dp


def warm_state(P, t0, seed):
    """The optimizer state a site starts from at counter t0: zeros at t0 = 0; otherwise m ~ N(0, 1e-3), v = 10^U(-12, -2)
    per element, and a 5 % stripe (every 20th element) left at m = v = 0."""
    m, v = np.zeros(P, np.float32), np.zeros(P, np.float32)
    if t0 > 0:
        rng = np.random.default_rng(seed)
        m = (rng.normal(size=P) * 1e-3).astype(np.float32)
        v = (10.0 ** rng.uniform(-12, -2, size=P)).astype(np.float32)
        m[::20] = 0
        v[::20] = 0
    return m, v


def worst(got, ref, bound):
    """(largest |got - ref| / bound, its index); a non-finite `got` counts as inf.  `ref` and `bound` must be finite: a NaN there
    would compare as met."""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound >= 0).all()
    diff = np.abs(got - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where((diff == 0) & (bound == 0), 0.0, diff / bound)      # (a bound of 0 met exactly)
    r = np.where(np.isfinite(got), r, np.inf)
    i = int(np.argmax(r))
    return float(r[i]), i
