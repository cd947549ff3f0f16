"""The shapes and data that tests/test_linprobe_cpu.py and tests/test_linprobe.py share (numpy only)."""
import functools

import numpy as np

import linprobe_ref as R

# (N, L, C): less than one tile and odd sizes; the default sizes with several tiles and a ragged last one; C past one wave and odd;
# the L gate with the smallest C; one labelled row; the C gate
SHAPES = [(203, 5, 3), (1031, 64, 10), (259, 7, 65), (300, 128, 2), (1, 1, 2), (4099, 16, 256)]
ITERS = [1, 50]
L2 = 1e-2
GATE = 1e-4          # every output tensor within GATE of its own maximum magnitude
MARGIN = 1e-4        # pred is compared where the reference's top two log-probs differ by more than this


def sid(shape):
    return "x".join(str(s) for s in shape)


@functools.lru_cache(maxsize=None)
def data(shape):
    """(x fp32 [N, L], y int32 [N] with 30 % of the rows -1) of a shape: separated Gaussian clusters.  Shared: not to be written to."""
    N, L, C = shape
    x, y, _ = R.clusters(N, L, C, seed=100 + SHAPES.index(shape), sep=4.0)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(shape, n_iter, l2=L2):
    """The statement's fit after n_iter iterations and its prediction on every row, computed once."""
    x, y = data(shape)
    f = R.fit(x, y, shape[2], l2, n_iter)
    f["predict"] = R.predict(x, f["W"], f["b"], y)
    return f


@functools.lru_cache(maxsize=None)
def overlapping(shape):
    """(x, y) for the comparison with scikit-learn: clusters that OVERLAP, as the classes of a latent code do -- centres of scale
    2 / sqrt(L), so about 2 sqrt(2) standard deviations apart whatever L -- with 30 % of the rows unlabelled.  (FISTA's O(1 / t^2)
    rate is in units of the solution's norm, which grows as the classes come apart: the well-separated `data` above, chosen for
    its margins, is after 300 iterations at f - f* = 1e-7 and 2e-6 where this one is at 1e-11 and 4e-10.)"""
    N, L, C = shape
    x, y, _ = R.clusters(N, L, C, seed=100 + SHAPES.index(shape), sep=2.0 / np.sqrt(L))
    return x, y


def margins(log_prob):
    """The gap between the two largest entries of each row."""
    top = np.sort(log_prob, axis=1)
    return top[:, -1] - top[:, -2]


def saturated(seed=7):
    """Separable codes scaled by 1e3: (x, y, C)."""
    x, y, _ = R.clusters(517, 9, 4, seed=seed, sep=6.0, scale=1e3)
    return x, y, 4
