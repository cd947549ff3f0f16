"""CPU-side checks of the chunked importance-weighted bound (include/gmvae_hip.h gmvae_iw_bound): declared, exported, bound,
its workspace sized by the chunk (not by n_samples), its argument checks, and the evaluation runner's flags.  No compute calls."""
import ctypes as C
import os
import re

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def test_header_declares_iw_bound(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gmvae_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(\w+)\s*\(", hdr))
    assert {"gmvae_iw_bound", "gmvae_iw_bound_workspace_bytes"} <= declared <= set(L.EXPORTS)
    assert L.lib.gmvae_abi_version() == 7


def _dims(L, B, chunk, row0=0, D=784, Lz=64, K=10, hidden=(64,)):
    d = L.make_dims(B, D, Lz, K, hidden, S=chunk)
    d.row0 = row0
    return d


def test_iw_workspace_holds_the_forward_and_grows_with_the_chunk(L):
    for model in (L.MODEL_GMVAE, L.MODEL_VAE, L.MODEL_VAE_GMP):
        d = _dims(L, 64, 50)
        assert L.iw_bound_workspace_bytes(d, model) > L.workspace_bytes(d, model)
        assert L.iw_bound_workspace_bytes(_dims(L, 64, 100), model) > L.iw_bound_workspace_bytes(d, model)


def test_iw_bound_argument_checks(L):
    d = _dims(L, 8, 5)
    p = C.c_void_p(1 << 20)                    # (never dereferenced: every check below fails before a launch)
    call = lambda dims, x=p, n=10, bound=None, ws=p: L.lib.gmvae_iw_bound(C.byref(dims), L.MODEL_GMVAE, x, p, n, bound, None, p,
                                                                           ws, 0, 0, None)
    assert call(d, n=0) == -2                                  # GMVAE_E_DIMS: no samples
    assert call(_dims(L, 8, 5, row0=(1 << 38) // 1000 - 7), n=1000) == -2      # (row0 + B) n >= 2^38: past the Philox row field
    assert call(d, x=C.c_void_p((1 << 20) + 4)) == -4         # GMVAE_E_ALIGN
    assert call(d, bound=C.c_void_p((1 << 20) + 8)) == -4
    assert call(d, ws=None) == -1                              # GMVAE_E_NULL
    assert call(_dims(L, 0, 5)) == -2


def test_eval_flags_iw_samples():
    from gmvae_amd import run_gmvae
    cfg = run_gmvae.build_parser().parse_args([])
    assert cfg.iw_samples == 0 and cfg.iw_chunk is None        # off by default: the reference's evaluation is unchanged
    cfg = run_gmvae.build_parser().parse_args(["--mode=eval", "--iw_samples=5000", "--iw_chunk=50"])
    assert cfg.iw_samples == 5000 and cfg.iw_chunk == 50
