"""The shapes and data that tests/test_twosample_cpu.py and tests/test_twosample.py share (numpy only).

A shape is (n, m, D, P): two samples of n and m rows of D dimensions pooled into N = n + m, and P splits.  Row 0 of the splits is
the observed one (the first n rows); where P allows, row 1 holds ONE point (n_p < 2: NaN), row 2 all but one (m_p < 2: NaN), row 3
n + 1 points (the rows may differ in size), row 4 a copy of row 0 and row 5 its complement (the ties the p-value must count); the
rest are random permutations' first n points."""
import functools

import numpy as np

import twosample_ref as R

# the kernel's tiles (csrc/twosample.hpp): 32 rows a workgroup, 64 columns a tile, 128 / 256 / 512 / 1024 splits a chunk, 32
# dimensions a chunk; below 256 row tiles the columns are cut into slabs
ISSUE = [(2, 2, 1, 1), (2, 3, 1, 4), (17, 15, 3, 5), (64, 64, 64, 16), (65, 63, 785, 17), (200, 131, 784, 33), (129, 127, 784, 257),
         (700, 837, 8, 64), (8, 8, 2, 200)]
EDGES = [(16, 15, 31, 1023), (16, 16, 32, 1024), (17, 16, 33, 1025),    # rows 31 / 32 / 33, dimensions 31 / 32 / 33, splits 1023 / 1024 / 1025 (two chunks)
         (32, 31, 5, 127), (32, 32, 5, 128), (33, 32, 5, 129),          # columns 63 / 64 / 65, splits 127 / 128 / 129
         (20, 13, 4, 255), (20, 14, 4, 256), (20, 15, 4, 257),          # splits 255 / 256 / 257
         (10, 9, 3, 511), (10, 10, 3, 512), (11, 10, 3, 513)]           # splits 511 / 512 / 513
SHAPES = ISSUE + EDGES
PIXELS, OFFSET, TIES = (200, 131, 784, 33), (129, 127, 784, 257), (8, 8, 2, 200)
VARIANTS = [("rbf", 1), ("rbf", 3), ("energy", 1), ("energy", 3)]      # (the energy kernel ignores Q)
DUPLICATES = [(0, 200), (1, 201), (2, 202), (3, 203), (4, 204), (5, 6)]      # PIXELS: five rows shared by the samples, one within


def sid(shape):
    return "x".join(str(s) for s in shape)


def vid(v):
    return f"{v[0]}{v[1]}"


@functools.lru_cache(maxsize=None)
def data(shape):
    """The pooled sample z [N, D] (fp32) of a shape."""
    n, m, D, P = shape
    rng = np.random.default_rng(1000 + 7 * n + 3 * m + D)
    if shape == PIXELS:
        z = np.concatenate([rng.random((n, D)) < 0.3, rng.random((m, D)) < 0.35]).astype(np.float32)
        for i, j in DUPLICATES:
            z[j] = z[i]
    elif shape == TIES:
        u, v = rng.standard_normal(D), rng.standard_normal(D)      # two distinct points: mmd2 depends on a split's count of u alone
        z = np.stack([u] * 6 + [v] * 2 + [u] * 2 + [v] * 6).astype(np.float32)
    else:
        z = np.concatenate([rng.standard_normal((n, D)), 0.3 + 1.2 * rng.standard_normal((m, D))]).astype(np.float32)
        if shape == OFFSET:
            z = (z + np.float32(1000.0)).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def splits(shape):
    n, m, D, P = shape
    N = n + m
    rng = np.random.default_rng(2000 + 7 * n + 3 * m + P)
    E = R.permutations(n, m, P, rng)
    special = [np.arange(N) == N // 2, np.arange(N) != N // 3, np.arange(N) < n + 1, np.arange(N) < n, np.arange(N) >= n]
    for p, row in enumerate(special, start=1):
        if p < P:
            E[p] = row
    E.setflags(write=False)
    return E


@functools.lru_cache(maxsize=None)
def sq_dists(shape):
    d2 = R.sq_dists(data(shape))
    d2.setflags(write=False)
    return d2


def gamma(shape, Q):
    """Bandwidths around the root-mean-square distance of the pooled rows."""
    sigma = R.kscale(data(shape), "energy")
    return R.gammas(sigma, (1.0,) if Q == 1 else (0.5, 1.0, 2.0))


@functools.lru_cache(maxsize=None)
def reference(shape, variant):
    """(mmd2 [P], row_all [N], row_first [N], kscale) of the statement."""
    kernel, Q = variant
    out = R.mmd(data(shape), splits(shape), kernel, gamma(shape, Q), d2=sq_dists(shape))
    return out + (R.kscale(data(shape), kernel),)
