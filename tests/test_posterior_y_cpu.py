"""CPU-side checks of the GMVAE's posterior over y by importance sampling per component (include/gmvae_hip.h
gmvae_posterior_y): declared, exported, bound, its workspace (the enumerated bound's plus the per-(row, component) fp64 state),
its argument checks (all before any launch) and the evaluation runner's flag.  No compute calls."""
import ctypes as C
import os
import re

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_posterior_y", "gmvae_posterior_y_workspace_bytes"}


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def test_header_declares_the_posterior(L):
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
    rc = L.lib.gmvae_posterior_y_workspace_bytes(C.byref(d), L.MODEL_GMVAE if model is None else model, C.byref(b))
    return rc, b.value


def test_workspace_holds_the_per_component_state_and_grows_with_the_chunk(L):
    for B, K in ((64, 10), (8, 80), (1, 1)):
        d = _dims(L, B, 5, K=K)
        small = L.posterior_y_workspace_bytes(d, L.MODEL_GMVAE)
        assert small >= L.iw_bound_enum_y_workspace_bytes(d, L.MODEL_GMVAE) + B * K * 24      # [B][K][3] doubles
        assert small % 16 == 0
        assert L.posterior_y_workspace_bytes(_dims(L, B, 10, K=K), L.MODEL_GMVAE) > small
        for flags in (L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW):                                  # the bits are ignored
            assert L.posterior_y_workspace_bytes(_dims(L, B, 5, K=K, flags=flags), L.MODEL_GMVAE) == small


def test_argument_checks(L):
    p = C.c_void_p(1 << 20)                    # (never dereferenced: every check below fails before a launch)

    def call(dims, model=None, x=p, n=10, lj=None, lp=None, stats=None, tail=p, ws=p, params=p):
        return L.lib.gmvae_posterior_y(C.byref(dims), L.MODEL_GMVAE if model is None else model, x, params, n, lj, lp, stats,
                                       tail, ws, 0, 0, None)

    d = _dims(L, 8, 5)
    assert call(d, n=0) == -2                                  # GMVAE_E_DIMS: no samples
    far = _dims(L, 8, 5, row0=(1 << 38) // 10000 - 7)          # (row0 + B) n K >= 2^38: past the Philox row field
    assert call(far, n=1000) == -2
    assert (far.row0 + 8) * 1000 < (1 << 38)
    big = _dims(L, 1 << 20, 1 << 7, K=16)                      # B S K = 2^31 > 2^30
    assert call(big) == -2 and _ws(L, big)[0] == -2
    for model in (L.MODEL_VAE, L.MODEL_VAE_GMP):               # GMVAE_E_MODEL: no y
        assert call(d, model=model) == -3 and _ws(L, d, model)[0] == -3
    off = C.c_void_p((1 << 20) + 4)
    assert call(d, x=off) == -4                                # GMVAE_E_ALIGN
    assert call(d, params=off) == -4
    assert call(d, lj=off) == -4
    assert call(d, lp=C.c_void_p((1 << 20) + 8)) == -4
    assert call(d, stats=off) == -4
    assert call(d, tail=off) == -4
    assert call(d, ws=off) == -4
    assert call(d, ws=None) == -1                              # GMVAE_E_NULL
    assert call(d, tail=None) == -1
    assert call(d, x=None) == -1
    assert call(d, params=None) == -1
    assert _ws(L, d)[0] == 0
    assert L.lib.gmvae_posterior_y_workspace_bytes(C.byref(d), L.MODEL_GMVAE, None) == -1
    assert call(_dims(L, 0, 5)) == -2
    assert call(_dims(L, 8, 0)) == -2


def test_eval_flag_posterior_samples():
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args([]))
    assert cfg.posterior_samples == 0                          # off by default: the reference's evaluation is unchanged
    for extra in ([], ["--y_inference=marginal"], ["--y_inference=marginal_iw", "--n_samples=3"]):
        cfg = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--posterior_samples=500", "--iw_chunk=5"] + extra))
        assert cfg.posterior_samples == 500 and cfg.iw_chunk == 5
    for model in ("vae", "vae_gmp"):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(["--mode=eval", f"--model={model}", "--posterior_samples=10"]))


def test_the_models_expose_the_posterior():
    from gmvae_amd.engine import Engine
    from gmvae_amd.gmvae import TrainableGMVAE
    assert callable(Engine.posterior_y)
    assert callable(TrainableGMVAE.posterior_y) and callable(TrainableGMVAE.predict_clusters)
