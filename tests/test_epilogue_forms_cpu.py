"""The table of tests/epilogue_cases.py without a device: a restatement of the tile classification of the loss epilogues
(csrc/gemm.hpp) holds the case table to "every (family, tile configuration, path) at least once", so that a later edit of the
shapes cannot silently lose a path; the "whole" shape is eligible for the big-round instance; every family's fp64 statement at
these shapes is finite and non-trivial."""
import os
import re

import numpy as np
import pytest

import epilogue_cases as EC
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(shape):
    sh = EC.SHAPES[shape]
    return sh.B * sh.d.S


def test_tile_classification():
    """The restatement on shapes small enough to count by hand."""
    assert EC.tile_paths(128, 256, 128, 128) == {"interior"}
    assert EC.tile_paths(128, 256, 32, 32) == {"interior"}
    assert EC.tile_paths(160, 272, 32, 32) == {"interior", "quad"}                 # 160 = 5 x 32: no ragged row at 32 x 32
    assert EC.tile_paths(160, 272, 64, 64) == {"interior", "quad", "ragged"}
    assert EC.tile_paths(32, 784, 32, 32) == {"interior", "quad"}                  # lik_ref's gumbel-784-* cases
    assert EC.tile_paths(16, 784, 32, 32) == {"ragged"}                            # pmask_ref's gumbel-784: no tile is whole
    assert EC.tile_paths(31, 64, 32, 32) == {"ragged"}
    assert EC.tile_paths(64, 30, 32, 32) == {"unaligned"}
    assert EC.tile_paths(64, 28, 32, 32) == {"quad"}
    assert EC.tile_paths(70, 135, 128, 128) == {"unaligned"}


def test_tile_sizes_are_the_kernels():
    """TILE against the configurations' template arguments in csrc/gemm.hpp and the size gates' text in gmvae_hip.hip."""
    src = open(os.path.join(ROOT, "gmvae_amd", "csrc", "gemm.hpp")).read()
    for cfg, name in ((0, "CfgS"), (1, "CfgM"), (2, "CfgL")):
        m = re.search(r"typedef\s+Cfg<\s*(\d+)\s*,\s*(\d+)\s*,[^>]*>\s*" + name + r"\s*;", src)
        assert m, name
        assert (int(m.group(1)), int(m.group(2))) == EC.TILE[cfg], name
    host = open(os.path.join(ROOT, "gmvae_amd", "csrc", "gmvae_hip.hip")).read()
    assert "p.M % 128 || p.N % 128" in host and "sg.K % 32" in host                # big_eligible's rules, restated in EC


@pytest.mark.parametrize("family", list(EC.FAMILIES))
@pytest.mark.parametrize("cfg", EC.CFGS)
def test_every_path_of_every_configuration_is_covered(family, cfg):
    BM, BN = EC.TILE[cfg]
    seen = set()
    for f, s in EC.STEP_CASES:
        if f == family:
            seen |= EC.tile_paths(_rows(s), EC.SHAPES[s].d.D, BM, BN)
    assert seen == set(EC.PATHS), (family, cfg, set(EC.PATHS) - seen)


def test_every_family_runs_every_gmvae_shape():
    for f in EC.FAMILIES:
        assert {s for g, s in EC.STEP_CASES if g == f} >= {"whole", "ragged", "unaligned"}
    for s in ("whole", "ragged", "unaligned"):
        assert EC.SHAPES[s].mname == "gmvae"
    for f in ("gauss-lsig", "gauss-f32-lsig"):
        assert {EC.SHAPES[s].mname for g, s in EC.STEP_CASES if g == f} == {"gmvae", "vae", "vae_gmp"}
    assert EC.SHAPES["ragged-vae_gmp-tanh"].d.act == "tanh"


def test_shapes_hold_what_their_names_say():
    w = EC.SHAPES["whole"]
    assert EC.big_round_eligible(_rows("whole"), w.d.D, w.d.hidden[-1]) and w.d.S > 1        # (the IWAE row weights are live)
    for cfg in EC.CFGS:
        assert EC.tile_paths(_rows("whole"), w.d.D, *EC.TILE[cfg]) == {"interior"}
        assert EC.tile_paths(_rows("ragged"), EC.SHAPES["ragged"].d.D, *EC.TILE[cfg]) == {"interior", "quad", "ragged"}
        assert EC.tile_paths(_rows("unaligned"), EC.SHAPES["unaligned"].d.D, *EC.TILE[cfg]) == {"unaligned"}
    assert not EC.big_round_eligible(_rows("ragged"), EC.SHAPES["ragged"].d.D, 64)
    # more than one row tile and more than one column tile in every configuration
    for s in ("ragged", "unaligned"):
        assert _rows(s) > 32 and EC.SHAPES[s].d.D > 128
    assert _rows("ragged") > 128


def test_forward_cases_cover_the_paths_without_a_c_output():
    """gmvae_forward's cases: the interior block, the predicated last column tile and the ragged rows under 64 x 64 and
    128 x 128, for one family per block of code (the masked Bernoulli, the byte likelihoods, the Gaussian's own block)."""
    assert {EC.FAMILIES[f].kind for f, _ in EC.FORWARD_CASES} == {"mask", "lik", "realx"}
    for f, s in EC.FORWARD_CASES:
        for cfg in EC.FORWARD_CFGS:
            assert EC.tile_paths(_rows(s), EC.SHAPES[s].d.D, *EC.TILE[cfg]) == {"interior", "quad", "ragged"}


@pytest.mark.parametrize("family,shape", EC.STEP_CASES, ids=[f"{f}-{s}" for f, s in EC.STEP_CASES])
def test_statement_is_finite_and_non_trivial(family, shape):
    I, (Cc, g) = EC.case(family, shape)
    fam = EC.FAMILIES[family]
    assert I.x.dtype == (np.float32 if fam.f32 else np.uint8) and I.x.shape == (I.B, I.d.D)
    assert I.flat.dtype == np.float32 and I.flat.shape[0] == O.pack(I.model, I.d, I.p32, np.float32).shape[0] + \
        (EC.RR.pad4(I.d.D) if fam.learned else 0)
    assert all(np.isfinite(Cc[k]) for k in ("loss", "nll", "kl", "nent")) and np.isfinite(Cc["rows"]).all()
    assert abs(Cc["loss"]) > 0 and abs(Cc["nll"]) > 0 and Cc["kl"] != 0
    for name, v in g.items():
        if name == EC.RR.LOG_SIGMA and not fam.learned:
            assert not v.any()
            continue
        assert np.isfinite(v).all() and np.abs(v).max() > 0, name
    if fam.kind == "mask":
        EC.PR.check_mask(I.mask)
        assert Cc["n_missing"] > 0 and Cc["n_observed"] > 0 and np.isfinite(Cc["hid"]) and Cc["hid"] != 0
    else:
        assert np.isfinite(Cc["sqerr"]) and Cc["sqerr"] > 0 and Cc["nll_abs"] > 0
    if I.d.S > 1:      # the row weights are live: the bound's weights within an example differ
        lw = Cc["rows"][:, 3].reshape(I.B, I.d.S)
        assert (lw.max(axis=1) - lw.min(axis=1)).min() > 0
