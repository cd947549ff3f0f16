"""CPU-side checks of the GMVAE's importance-weighted bound with y summed out over K (include/gmvae_hip.h
gmvae_iw_bound_enum_y): declared, exported, bound, its workspace sized by the chunk, its argument checks (all before any
launch) and the evaluation runner's flag.  No compute calls."""
import ctypes as C
import os
import re

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_iw_bound_enum_y", "gmvae_iw_bound_enum_y_workspace_bytes"}


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def test_header_declares_the_enumerated_bound(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmvae_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(\w+)\s*\(", hdr))
    assert NAMES <= declared <= set(L.EXPORTS)
    for name in NAMES:
        assert hasattr(L.lib, name)
    assert L.lib.gmvae_abi_version() == 7


def _dims(L, B, chunk, row0=0, K=10, flags=0, D=784, Lz=64, hidden=(64,)):
    d = L.make_dims(B, D, Lz, K, hidden, S=chunk, sched_flags=flags)
    d.row0 = row0
    return d


def _ws(L, d, model=None):
    b = C.c_uint64()
    rc = L.lib.gmvae_iw_bound_enum_y_workspace_bytes(C.byref(d), L.MODEL_GMVAE if model is None else model, C.byref(b))
    return rc, b.value


def test_workspace_grows_with_the_chunk_and_ignores_the_marginal_bit(L):
    d = _dims(L, 64, 5)
    small = L.iw_bound_enum_y_workspace_bytes(d, L.MODEL_GMVAE)
    assert small > L.workspace_bytes(_dims(L, 64, 1, flags=L.OBJ_MARGINAL_Y), L.MODEL_GMVAE)     # B*K rows < B*5*K rows
    assert L.iw_bound_enum_y_workspace_bytes(_dims(L, 64, 10), L.MODEL_GMVAE) > small
    assert L.iw_bound_enum_y_workspace_bytes(_dims(L, 64, 5, flags=L.OBJ_MARGINAL_Y), L.MODEL_GMVAE) == small


def test_argument_checks(L):
    p = C.c_void_p(1 << 20)                    # (never dereferenced: every check below fails before a launch)

    def call(dims, model=None, x=p, n=10, bound=None, ws=p):
        return L.lib.gmvae_iw_bound_enum_y(C.byref(dims), L.MODEL_GMVAE if model is None else model, x, p, n, bound, None, p,
                                           ws, 0, 0, None)

    d = _dims(L, 8, 5)
    assert call(d, n=0) == -2                                  # GMVAE_E_DIMS: no samples
    # (row0 + B) n K >= 2^38: past the Philox row field (the Gumbel bound's (row0 + B) n would still fit)
    far = _dims(L, 8, 5, row0=(1 << 38) // 10000 - 7)
    assert call(far, n=1000) == -2
    assert (far.row0 + 8) * 1000 < (1 << 38)
    big = _dims(L, 1 << 20, 1 << 7, K=16)                      # B S K = 2^31 > 2^30 (B S = 2^27 passes check_dims)
    assert call(big) == -2 and _ws(L, big)[0] == -2
    for model in (L.MODEL_VAE, L.MODEL_VAE_GMP):               # GMVAE_E_MODEL: no y to sum out
        assert call(d, model=model) == -3 and _ws(L, d, model)[0] == -3
    assert call(d, x=C.c_void_p((1 << 20) + 4)) == -4         # GMVAE_E_ALIGN
    assert call(d, bound=C.c_void_p((1 << 20) + 8)) == -4
    assert call(d, ws=None) == -1                              # GMVAE_E_NULL
    assert call(_dims(L, 0, 5)) == -2
    assert call(_dims(L, 8, 0)) == -2
    # the Gumbel bound still refuses the marginal bit
    assert L.lib.gmvae_iw_bound(C.byref(_dims(L, 8, 1, flags=L.OBJ_MARGINAL_Y)), L.MODEL_GMVAE, p, p, 10, None, None, p, p,
                                0, 0, None) == -2


def test_eval_flag_iw_enum_samples():
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args([]))
    assert cfg.iw_enum_samples == 0                            # off by default: the reference's evaluation is unchanged
    for extra in ([], ["--y_inference=marginal"]):
        cfg = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--iw_enum_samples=500", "--iw_chunk=5"] + extra))
        assert cfg.iw_enum_samples == 500 and cfg.iw_chunk == 5
    for model in ("vae", "vae_gmp"):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(["--mode=eval", f"--model={model}", "--iw_enum_samples=10"]))
    with pytest.raises(SystemExit):                            # unchanged: the Gumbel bound is not the marginal objective's
        run_gmvae.check_args(p, p.parse_args(["--y_inference=marginal", "--iw_samples=10"]))
