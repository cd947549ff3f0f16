"""The shapes, data and gates that tests/test_pca_cpu.py and tests/test_pca.py share (numpy only)."""
import functools

import numpy as np

import pca_ref as R

# (N, D, k): the smallest sizes; N off every tile multiple; D off 16 and off 64; k < D; the gate's edge
DENSE = [(2, 1, 1), (37, 3, 3), (500, 24, 24), (403, 64, 10), (333, 100, 100), (1031, 128, 128)]
# (N, D, k, m): just past the gate; the notes' case; N < D; D off 64 with more than one macro-block row
ITERATIVE = [(257, 129, 4, 20), (600, 200, 8, 16), (300, 784, 16, 32), (150, 1040, 4, 12)]
EIGH_SIZES = [1, 2, 3, 17, 128]

# the defaults of gmvae_amd.pca, pinned on the statement (tests/test_pca_cpu.py; profiles/pca_notes.md)
N_SWEEPS = 15
N_ITER = 60
OVERSAMPLE = 8

GATE = 1e-9           # mean, explained_variance, total_variance, residual (in units of lambda_1): of the tensor's own max |ref|
GATE_COMPONENTS = 1e-8
GATE_OFFDIAG = 1e-12
GATE_TRANSFORM = 1e-6
MIN_GAP = 1e-6        # a component is compared where its eigenvalue is this far, relative to lambda_1, from its neighbours'
SWEEP_TARGET = 1e-13  # n_sweeps: the smallest count that leaves offdiag below this on every n = 128 fixture, plus three
RESIDUAL_TARGET = 1e-10


def sid(shape):
    return "x".join(str(s) for s in shape)


def _decay(D):
    return 0.95 if D >= 64 else 0.8


@functools.lru_cache(maxsize=None)
def data(shape):
    """x fp32 [N, D] of a table row: a decaying spectrum in a random basis, offset by a standard normal vector.  Not to be written to."""
    N, D = shape[:2]
    return R.fixture(N, D, decay=_decay(D) if len(shape) == 3 else 0.9, seed=200 + (DENSE + ITERATIVE).index(shape))


@functools.lru_cache(maxsize=None)
def start(shape):
    """The orthonormal start V0 [D, m] of an iterative row."""
    return R.start(shape[1], shape[3], seed=300 + ITERATIVE.index(shape))


@functools.lru_cache(maxsize=None)
def reference(shape, n_iter=N_ITER):
    """The statement's fit of a table row, computed once."""
    if len(shape) == 3:
        return R.fit(data(shape), shape[2])
    return R.fit(data(shape), shape[2], shape[3], n_iter, start(shape))


@functools.lru_cache(maxsize=None)
def big_offset():
    """An offset of 1e4 on data of variance about one: the expanded square would lose eight of fp64's sixteen digits."""
    return (R.fixture(300, 16, decay=0.8, seed=231, offset=0.0) + np.float32(1e4)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def constant_column():
    x = R.fixture(211, 6, decay=0.8, seed=232)
    x[:, 3] = 2.5
    return x


@functools.lru_cache(maxsize=None)
def equal_rows():
    return np.tile(R.fixture(1, 5, seed=233), (77, 1))


RANK_DEFICIENT = (300, 200, 8, 16)      # rank 10 below m = 16: the factorisation of G meets a pivot that is not > 0 at index 10 .. 15


@functools.lru_cache(maxsize=None)
def rank_deficient():
    """(x, V0): rows in a 10-dimensional subspace, EXACTLY in fp32 (small integers), so that G = W^T W has rank 10."""
    rng = np.random.default_rng(234)
    N, D = RANK_DEFICIENT[:2]
    x = (rng.integers(-8, 9, (N, 10)) @ rng.integers(-4, 5, (10, D))).astype(np.float32)
    return x, R.start(D, RANK_DEFICIENT[3], seed=334)


def gaps(var_all, k):
    """The distance of each of the first k eigenvalues from its neighbours', relative to the largest."""
    w = np.asarray(var_all, dtype=np.float64)
    d = np.abs(np.diff(w))
    left = np.concatenate(([np.inf], d))[:k]
    right = np.concatenate((d, [np.inf]))[:k]
    return np.minimum(left, right) / w[0]


def sign_margin(comp):
    """The gap between the two largest |entries| of each row (inf for a row of one entry)."""
    a = np.sort(np.abs(comp), axis=1)
    return a[:, -1] - a[:, -2] if a.shape[1] > 1 else np.full(len(a), np.inf)


def sym(n, seed):
    """A symmetric test matrix [n, n] with a spread spectrum."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    return (Q * (0.9 ** np.arange(n) * np.where(np.arange(n) % 3 == 2, -1.0, 1.0))) @ Q.T
