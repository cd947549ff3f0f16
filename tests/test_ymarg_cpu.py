"""CPU side of the enumerated-y GMVAE objective (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y): the fp64 statement
(tests/ymarg_ref.py) against the oracle where the two objectives coincide (K = 1), its logits gradient against the closed
form the kernels use, the flag in the header / _lib / the argument checks of the C ABI, the factory and the runner's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import ymarg_ref as YM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def _setup(d, B, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:                                   # non-zero biases: every term of the gradient is exercised
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.1, p[k].shape)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * d.K, d.L))
    return p, x, eps


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_k1_equals_the_oracle_at_one_sample(act):
    """K = 1: the relaxed y of the Gumbel objective is exactly [1], q(y|x) = 1 and nent = 0 -- both objectives are the
    single-sample ELBO, for any u."""
    d = O.Dims(D=30, L=3, K=1, hidden=(12, 9), act=act)
    B = 5
    p, x, eps = _setup(d, B)
    u = np.random.default_rng(3).uniform(0.01, 0.99, (B, 1))
    Cm, gm = YM.loss_and_grads(d, p, x, eps)
    Co, go = O.loss_and_grads(O.MODEL_GMVAE, d, p, x, eps, u, np.float64)
    for k in ("loss", "nll", "kl", "nent"):
        assert abs(Cm[k] - Co[k]) <= 1e-10 * max(1.0, abs(Co[k])), k
    for name, ref in go.items():
        np.testing.assert_allclose(gm[name], ref, rtol=1e-9, atol=1e-12, err_msg=name)


def test_logits_gradient_is_the_closed_form():
    d = O.Dims(D=40, L=4, K=6, hidden=(16,))
    B = 7
    p, x, eps = _setup(d, B, seed=2)
    Cm, _ = YM.loss_and_grads(d, p, x, eps)
    np.testing.assert_allclose(Cm["dlogits"], YM.dlogits_closed_form(Cm, B), rtol=1e-9, atol=1e-13)
    # and the loss is the q-weighted sum of the row terms plus the entropy
    q, rows = Cm["q"], Cm["rows"].reshape(B, d.K, 4)
    lb = (q * np.log(q)).sum(1) - (q * rows[..., 3]).sum(1)
    assert abs(lb.mean() - Cm["loss"]) <= 1e-10 * abs(Cm["loss"])


def test_relu_masks_take_the_given_subgradient():
    d = O.Dims(D=20, L=3, K=3, hidden=(8,))
    B = 4
    p, x, eps = _setup(d, B, seed=4)
    C0, g0 = YM.loss_and_grads(d, p, x, eps)
    masks = {net: [None] + [pre > 0 for pre, _ in C0["pre"][net]] for net in C0["pre"]}
    _, g1 = YM.loss_and_grads(d, p, x, eps, relu_masks=masks)           # the fp64 masks themselves: same gradients
    for k in g0:
        np.testing.assert_allclose(g1[k], g0[k], rtol=1e-12, atol=1e-15)
    masks["decoder"][1] = np.zeros_like(masks["decoder"][1])            # a closed layer: no gradient below it
    _, g2 = YM.loss_and_grads(d, p, x, eps, relu_masks=masks)
    assert not g2["decoder_fcnet/linear_0/w"].any()


def test_header_flag_matches_lib(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    m = re.search(r"GMVAE_OBJ_MARGINAL_Y\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == L.OBJ_MARGINAL_Y == 4
    assert L.OBJ_MARGINAL_Y & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID) == 0


def _mdims(L, B=16, K=10, S=1, flags=None):
    return L.make_dims(B, 784, 8, K, (64,), S=S, sched_flags=L.OBJ_MARGINAL_Y if flags is None else flags)


def test_abi_checks_and_workspace(L):
    for model in (L.MODEL_VAE, L.MODEL_VAE_GMP):
        assert L.lib.gmvae_workspace_bytes(C.byref(_mdims(L)), model, C.byref(C.c_uint64())) == -3       # GMVAE_E_MODEL
    assert L.lib.gmvae_workspace_bytes(C.byref(_mdims(L, S=2)), L.MODEL_GMVAE, C.byref(C.c_uint64())) == -2
    assert L.lib.gmvae_workspace_bytes(C.byref(_mdims(L, B=1 << 27, K=16)), L.MODEL_GMVAE, C.byref(C.c_uint64())) == -2
    assert L.lib.gmvae_iw_bound_workspace_bytes(C.byref(_mdims(L)), L.MODEL_GMVAE, C.byref(C.c_uint64())) == -2
    # the workspace holds B*K rows: at least the general schedule's buffers of the Gumbel step at S = K
    assert L.workspace_bytes(_mdims(L), L.MODEL_GMVAE) >= L.workspace_bytes(_mdims(L, S=10, flags=0), L.MODEL_GMVAE)
    # the per-row buffers hold B*K rows: offsets equal the S = K layout's
    for name in (b"hg1", b"hd1", b"z", b"logw", b"dqp"):
        o1, o2 = C.c_uint64(), C.c_uint64()
        L.check(L.lib.gmvae_workspace_offset(C.byref(_mdims(L)), L.MODEL_GMVAE, name, C.byref(o1)), "offset")
        L.check(L.lib.gmvae_workspace_offset(C.byref(_mdims(L, S=10, flags=0)), L.MODEL_GMVAE, name, C.byref(o2)), "offset")
        assert o1.value == o2.value, name
    # parameters do not depend on the objective
    assert L.param_layout(_mdims(L), L.MODEL_GMVAE) == L.param_layout(_mdims(L, flags=0), L.MODEL_GMVAE)


def test_schedule_names(L):
    assert L.step_schedule(_mdims(L), L.MODEL_GMVAE) == "general+marginal"
    cfg2 = L.make_dims(1024, 784, 64, 10, (64,))
    cfg2m = L.make_dims(1024, 784, 64, 10, (64,), sched_flags=L.OBJ_MARGINAL_Y)
    assert L.step_schedule(cfg2m, L.MODEL_GMVAE).startswith("general+marginal")
    assert "marginal" not in L.step_schedule(cfg2, L.MODEL_GMVAE)


def test_factory_rejects_unknown_mode(L):
    from gmvae_amd import gmvae
    from gmvae_amd.engine import Engine
    with pytest.raises(ValueError, match="y_inference"):
        gmvae.create_gmvae(784, 8, mixture_components=10, y_inference="x")
    with pytest.raises(ValueError, match="marginal"):
        Engine("vae", 784, 8, 1, [64], y_inference="marginal")
    with pytest.raises(ValueError, match="marginal"):
        gmvae.create_gmvae(784, 8, mixture_components=10, n_samples=2, y_inference="marginal")
    import inspect
    from gmvae_amd import vae
    assert "y_inference" not in inspect.signature(vae.create_vae).parameters


def test_runner_flag(L):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    assert p.parse_args([]).y_inference == "gumbel"
    assert p.parse_args(["--y_inference=marginal"]).y_inference == "marginal"
    for bad in (["--y_inference=x"], ["--y_inference=marginal", "--iw_samples=10"],
                ["--y_inference=marginal", "--model=vae"], ["--y_inference=marginal", "--n_samples=3"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    cfg = run_gmvae.check_args(p, p.parse_args(["--y_inference=marginal", "--mode=eval"]))
    assert cfg.y_inference == "marginal"
