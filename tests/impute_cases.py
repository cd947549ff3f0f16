"""The cases of tests/test_impute_cpu.py and tests/test_impute.py: pmask_ref.setup's shapes and masks (a row that observes
nothing, a row that misses only the dead columns, the last column dead; x flipped at the missing pixels), each at the sample
counts and chunks that reach every path of the fold -- a partial last chunk and blocks shorter than 16 rows, a whole 16-row block
plus a partial one, one chunk, and a single sample."""
import numpy as np

import impute_ref as IR
import pmask_ref as PR

SEED, STEP = 5, 3
M_DRAWS = 5                     # two quads of the u stream: columns 4 ceil(K / 4) .. + 4
CASES = ("vae", "vae_gmp", "gumbel", "gumbel-d99", "gumbel-784", "vae-saturated")
RUNS = ((7, 3), (40, 16), (40, 40))          # (n, chunk)
PARAMS = [(c, n, ch) for c in CASES for (n, ch) in RUNS] + [("gumbel", 1, 1)]

# The gate on mean_out against the statement on the DEVICE's log w and the reference's logits (test 2).  Measured on the CPU over
# all PARAMS (tests/test_impute_cpu.py re-measures and asserts it): the same statement in fp32 torch, layer products included,
# against the fp64 one differs by at most FP32_FLOOR; the device sums three layers and the exponentials in another order: 16 x.
FP32_FLOOR = 3.8e-7
MEAN_GATE = max(16 * FP32_FLOOR, 1e-6)
MAX_LEFT_OUT = 0.10             # the share of draws whose two best keys are too close to compare

_STATE = {}


def setup(name):
    """pmask_ref.setup(name), once."""
    if ("setup", name) not in _STATE:
        _STATE["setup", name] = PR.setup(name)
    return _STATE["setup", name]


def statement(name, n, masked=True, row0=0):
    """(samples, estimate) of the fp64 statement for the case at n samples: computed once, shared, left unchanged."""
    key = (name, n, masked, row0)
    if key not in _STATE:
        model, d, p32, flat, xf, eps, u, m, x = setup(name)
        s = IR.samples(model, d, p32, xf, m if masked else None, n, M_DRAWS, SEED, STEP, row0)
        e = IR.estimate(s["lw"], s["lam"], s["hid"], s["g"], s["z"])
        for v in list(s.values()) + [v for v in e.values()]:
            v.setflags(write=False)
        _STATE[key] = (s, e)
    return _STATE[key]
