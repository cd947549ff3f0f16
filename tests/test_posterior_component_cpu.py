"""CPU-side checks of the VAE_GMP's posterior over the component of its mixture prior by importance sampling (include/gmvae_hip.h
gmvae_posterior_component): declared, exported, bound, its workspace (the streamed bound's plus the per-(row, component) fp64
state), its argument checks (all before any launch), the evaluation runner's flag, and the fp64 reference the GPU tests use.  No
compute calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_posterior_component", "gmvae_posterior_component_workspace_bytes"}


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
    rc = L.lib.gmvae_posterior_component_workspace_bytes(C.byref(d), L.MODEL_VAE_GMP if model is None else model, C.byref(b))
    return rc, b.value


def test_workspace_holds_the_per_component_state_and_grows_with_the_chunk(L):
    for B, K, Lz in ((64, 10, 64), (8, 80, 8), (1, 1, 8), (16, 7, 5)):
        d = _dims(L, B, 5, K=K, Lz=Lz)
        small = L.posterior_component_workspace_bytes(d, L.MODEL_VAE_GMP)
        assert small >= L.iw_bound_workspace_bytes(d, L.MODEL_VAE_GMP) + B * K * 16           # [B][K][2] doubles
        assert small % 16 == 0
        assert L.posterior_component_workspace_bytes(_dims(L, B, 10, K=K, Lz=Lz), L.MODEL_VAE_GMP) > small


def test_argument_checks(L):
    p = C.c_void_p(1 << 20)                    # (never dereferenced: every check below fails before a launch)

    def call(dims, model=None, x=p, n=10, lj=None, lp=None, stats=None, tail=p, ws=p, params=p):
        return L.lib.gmvae_posterior_component(C.byref(dims), L.MODEL_VAE_GMP if model is None else model, x, params, n, lj, lp,
                                               stats, tail, ws, 0, 0, None)

    d = _dims(L, 8, 5)
    assert call(d, n=0) == -2                                  # GMVAE_E_DIMS: no samples
    far = _dims(L, 8, 5, row0=(1 << 38) // 1000 - 7)           # (row0 + B) n >= 2^38: past the Philox row field
    assert call(far, n=1000) == -2
    near = _dims(L, 8, 5, row0=(1 << 38) // 1000 - 9)          # ... and just inside it the next check is reached
    assert (near.row0 + 8) * 1000 < (1 << 38) and call(near, n=1000, ws=None) == -1
    big = _dims(L, 1 << 20, 1 << 11)                           # B S = 2^31 > 2^30
    assert call(big) == -2 and _ws(L, big)[0] == -2
    for model in (L.MODEL_VAE, L.MODEL_GMVAE):                 # GMVAE_E_MODEL: the VAE_GMP's alone
        assert call(_dims(L, 8, 5, K=1 if model == L.MODEL_VAE else 10), model=model) == -3
        assert _ws(L, d, model)[0] == -3
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
    assert L.lib.gmvae_posterior_component_workspace_bytes(C.byref(d), L.MODEL_VAE_GMP, None) == -1
    assert call(_dims(L, 0, 5)) == -2
    assert call(_dims(L, 8, 0)) == -2


def test_eval_flag_component_posterior_samples():
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args([]))
    assert cfg.component_posterior_samples == 0                # off by default: the reference's evaluation is unchanged
    cfg = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--model=vae_gmp", "--component_posterior_samples=500",
                                                "--iw_chunk=5"]))
    assert cfg.component_posterior_samples == 500 and cfg.iw_chunk == 5
    for model in ("vae", "gmvae"):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(["--mode=eval", f"--model={model}", "--component_posterior_samples=10"]))
    with pytest.raises(SystemExit):                            # evaluation only
        run_gmvae.check_args(p, p.parse_args(["--mode=train", "--model=vae_gmp", "--component_posterior_samples=10"]))
    with pytest.raises(SystemExit):                            # --posterior_samples keeps refusing the VAE family
        run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--model=vae_gmp", "--posterior_samples=10"]))


def test_the_models_expose_the_posterior():
    from gmvae_amd.engine import Engine
    from gmvae_amd.vae import TrainableVAE
    assert callable(Engine.posterior_component)
    assert callable(TrainableVAE.posterior_component) and callable(TrainableVAE.predict_clusters)


def test_the_fp64_reference_is_the_oracles_bound_and_stays_finite_for_a_separated_mixture():
    """tests/post_comp_ref.py: logsumexp_k log w_sk is the oracle's own log w, and with the mixture pulled apart (most components
    thousands of nats below the logsumexp, where a responsibility is 0 in fp64 too) every log w_sk is still finite."""
    import dataclasses
    import oracle as O
    import post_comp_ref as R
    d = O.Dims(D=100, L=5, K=7, hidden=(24, 24))
    flat = O.pack(O.MODEL_VAE_GMP, d, O.init_params(O.MODEL_VAE_GMP, d, np.random.default_rng(0)), np.float32)
    x, _, _ = O.make_inputs(d, 3, O.MODEL_VAE_GMP, seed_x=100)
    n = 6
    for f in (flat, R.separate(d, flat)):
        lw = R.log_w(d, f, x, n, 2, 11, 3)
        assert lw.shape == (3, n, d.K) and np.all(np.isfinite(lw))
        p64 = O.unpack(O.MODEL_VAE_GMP, d, f.astype(np.float64))
        for b in range(3):
            eps, _ = O.noise(n, d.L, d.K, (2 + b) * n, 11, 3)
            Cb = O.forward(O.MODEL_VAE_GMP, dataclasses.replace(d, S=n), p64, x[b:b + 1], eps, None)
            np.testing.assert_allclose(R.lse(lw[b], axis=1), Cb["logw"], rtol=1e-12)
            np.testing.assert_allclose(R.statement(lw)["bound"][b], Cb["bound"][0], rtol=1e-12)
    far = R.log_w(d, R.separate(d, flat), x, n, 2, 11, 3)
    gap = far - R.lse(far, axis=2)[:, :, None]
    assert (gap < -1000).mean() > 0.5                          # most components: far below where exp underflows
    s = R.statement(far)
    assert all(np.all(np.isfinite(v)) for v in s.values())
