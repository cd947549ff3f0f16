"""The shapes and data that tests/test_sinkhorn_cpu.py and tests/test_sinkhorn.py share (numpy only).

A shape is (n, m, D, T): two samples of n and m rows of D dimensions and T iterations; every shape runs with uniform weights and
with random positive ones, at blur_rel = 0.2 and n_final = T // 4.  They are the smallest shapes that cross every edge of the
kernel's tiles (csrc/sinkhorn.hpp): 32 rows a workgroup, 64 columns a tile, 32 dimensions a chunk, the columns cut into slabs below
256 row tiles of the larger sample."""
import functools
import os

import numpy as np

import sinkhorn_ref as R

TABLE = [(1, 1, 1, 3), (1, 5, 2, 4), (2, 3, 1, 12), (31, 33, 3, 12), (32, 64, 31, 12), (33, 65, 32, 12), (65, 63, 33, 12),
         (129, 97, 64, 12)]                    # the error-table shapes
OFFSET = (129, 127, 785, 12)                   # every row shifted by 1000: the centring
PIXELS = (200, 131, 784, 12)                   # 0 / 1 rows, five shared between the samples and one pair equal within a sample
SINGLE_SLAB = (8200, 70, 4, 3)                 # 257 row tiles: one slab; few columns
SHAPES = TABLE + [OFFSET, PIXELS, SINGLE_SLAB]
WEIGHTS = ["uniform", "random"]
DUPLICATES = [(0, 200), (1, 201), (2, 202), (3, 203), (4, 204), (5, 6)]      # PIXELS, pooled rows
BLUR_REL = 0.2


def sid(shape):
    return "x".join(str(s) for s in shape)


@functools.lru_cache(maxsize=None)
def data(shape):
    """(x [n, D], y [m, D]) in fp32."""
    n, m, D, T = shape
    rng = np.random.default_rng(3000 + 7 * n + 3 * m + D)
    if shape == PIXELS:
        z = np.concatenate([rng.random((n, D)) < 0.3, rng.random((m, D)) < 0.35]).astype(np.float32)
        for i, j in DUPLICATES:
            z[j] = z[i]
    else:
        z = np.concatenate([rng.standard_normal((n, D)), 0.3 + 1.2 * rng.standard_normal((m, D))]).astype(np.float32)
        if shape == OFFSET:
            z = (z + np.float32(1000.0)).astype(np.float32)
    z.setflags(write=False)
    return z[:n], z[n:]


@functools.lru_cache(maxsize=None)
def weights(shape, kind):
    """(a [n], b [m]) in fp64, normalised; (None, None) for the uniform ones."""
    if kind == "uniform":
        return None, None
    n, m, D, T = shape
    rng = np.random.default_rng(4000 + 7 * n + 3 * m + D)
    a, b = rng.uniform(0.2, 1.8, n), rng.uniform(0.2, 1.8, m)
    a, b = a / a.sum(), b / b.sum()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def eps(shape):
    n, m, D, T = shape
    out = R.schedule(np.concatenate(data(shape)), T, blur_rel=BLUR_REL, n_final=T // 4)
    out.setflags(write=False)
    return out


def scale(shape):
    return R.cscale(np.concatenate(data(shape)))


def recorded(kind):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sinkhorn", f"single_slab_{kind}.npz")


@functools.lru_cache(maxsize=None)
def reference(shape, kind, form="statement"):
    """The statement's dict (form="expanded": the device's form in fp64) on a shape; computed once, not to be changed.  The
    statement on SINGLE_SLAB -- seven passes over 8200 x 8200 costs in longdouble, 45 s -- is a recorded result
    (`python tests/sinkhorn_cases.py` writes it); tests/test_sinkhorn_cpu.py holds it against the fp64 form, computed afresh."""
    x, y = data(shape)
    a, b = weights(shape, kind)
    if shape == SINGLE_SLAB and form == "statement" and os.path.exists(recorded(kind)):
        with np.load(recorded(kind)) as z:
            out = {k: z[k] for k in ("f", "g", "p", "q")}
            out.update({k: float(z[k]) for k in ("sinkhorn", "part_x", "part_y", "marginal_err")})
        out["contrib_x"], out["contrib_y"] = out["f"] - out["p"], out["g"] - out["q"]
        return out
    return R.divergence(x, y, eps(shape), a, b, form=form)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(recorded("uniform")), exist_ok=True)
    for kind in WEIGHTS:
        if os.path.exists(recorded(kind)):
            os.remove(recorded(kind))
        ref = reference(SINGLE_SLAB, kind)
        np.savez(recorded(kind), **{k: ref[k] for k in ("f", "g", "p", "q", "sinkhorn", "part_x", "part_y", "marginal_err")})
        print(recorded(kind), ref["sinkhorn"])
