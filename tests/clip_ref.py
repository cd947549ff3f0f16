"""The fp64 statement of GMVAE_OPT_CLIP_NORM (include/gmvae_hip.h) and the bounds the device is held to.

With g the gradient SUMS buf[0, P), count = buf[P + 4], the loss sum buf[P], SS = sum_i g_i^2 and C the threshold:
    norm = sqrt(SS) / count                 the global norm of the mean gradient, before clipping
    d    = max(count, sqrt(SS) / C)         g_i / d = (g_i / count) min(1, C / norm)
and the step is skipped unless C > 0, SS is finite and the loss sum is finite.

Bounds (derived, not measured).  The device sums exact fp64 squares in fp64: a relative error of at most n 2^-53 on SS, <= 1e-9
for n <= 1e7 elements, so <= 5e-10 on its root.  sqrt, the division by (double)C and the max run in fp64 (2^-53 each), then ONE
rounding to fp32, u = 2^-24.  Hence |norm_dev - norm| <= 2 u norm and |d_dev - d| <= 2 u d: one u is the rounding, one is slack
that covers the 5e-10 (u = 6e-8) a hundred times over.  d is continuous in C, so the bound on d also holds where the norm is
within rounding of C; only the FLAG may go either way there, when |sqrt(SS) / C - count| <= 2 u count (flag_band)."""
import math

import numpy as np

U = 2.0 ** -24
TAIL = 8


def record(buf, C):
    """(norm, d, clipped, skip) of a gradient buffer [P + TAIL] (any float dtype; read as the fp32 values it holds) at the
    threshold C.  Under skip only `skip` is specified: the other three are what the formulas give (possibly inf / NaN)."""
    b = np.asarray(buf, dtype=np.float32).astype(np.float64)
    P = b.shape[0] - TAIL
    g, loss, count = b[:P], b[P], b[P + 4]
    C = float(np.float32(C))
    with np.errstate(all="ignore"):
        ss = float(np.sum(g * g))
        root = math.sqrt(ss) if ss >= 0 and math.isfinite(ss) else ss
        skip = not (C > 0.0) or not math.isfinite(ss) or not math.isfinite(loss)
        over = root / C if C != 0.0 else (math.inf if root > 0 else math.nan)
        d = over if over > count else count
        norm = root / count
    return norm, d, bool(not skip and over > count), skip


def flag_band(buf, C):
    """True where the clipped flag may go either way: sqrt(SS) / C within 2 u count of count."""
    b = np.asarray(buf, dtype=np.float32).astype(np.float64)
    P = b.shape[0] - TAIL
    count = b[P + 4]
    over = math.sqrt(float(np.sum(b[:P] * b[:P]))) / float(np.float32(C))
    return abs(over - count) <= 2 * U * count


def clipped_mean_gradient(buf, C):
    """What Adam is fed: g / d, in fp64 (None for a skipped step)."""
    b = np.asarray(buf, dtype=np.float32).astype(np.float64)
    P = b.shape[0] - TAIL
    _, d, _, skip = record(buf, C)
    return None if skip else b[:P] / d


def check_record(rec, buf, C):
    """Holds a device record [4] (fp32) to the statement; returns the worst |device - fp64| / bound over norm and d (0 for a
    skipped step) for the notes."""
    rec = np.asarray(rec, dtype=np.float32)
    norm, d, clipped, skip = record(buf, C)
    if skip:
        assert np.isnan(rec[3]), ("a skipped step carries a NaN guard", rec)
        return 0.0
    loss = np.asarray(buf, dtype=np.float32)[-TAIL]
    assert rec[3] == loss, ("the guard is the loss sum", rec, loss)
    worst = 0.0
    for name, got, want in (("norm", rec[0], norm), ("d", rec[1], d)):
        bound = 2 * U * abs(want)
        err = abs(float(got) - want)
        assert err <= bound, (name, float(got), want, err / U / max(abs(want), 1e-300))
        worst = max(worst, err / bound if bound > 0 else 0.0)
    assert rec[2] in (0.0, 1.0)
    if not flag_band(buf, C):
        assert bool(rec[2]) == clipped, ("clipped flag", rec, norm, C)
    return worst
