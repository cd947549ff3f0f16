"""CPU side of the importance-weighted objective with y summed out (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y_IW): the fp64
statement (tests/ymarg_iw_ref.py) against the S = 1 marginal statement and central differences, the bound sandwich
mean_logw <= -L <= bound, the flag in the header / _lib, the argument checks of the C ABI, the factory and the runner's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import ymarg_iw_ref as YI
import ymarg_ref as YM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def _setup(d, B, S, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:                                   # non-zero biases: every term of the gradient is exercised
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.1, p[k].shape)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * S * d.K, d.L))
    return p, x, eps


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_one_sample_is_the_marginal_statement(act):
    d = O.Dims(D=30, L=3, K=4, hidden=(12, 9), act=act)
    B = 5
    p, x, eps = _setup(d, B, 1)
    Ci, gi = YI.loss_and_grads(d, p, x, eps, 1)
    Cm, gm = YM.loss_and_grads(d, p, x, eps)
    for k in ("loss", "nll", "kl", "nent"):
        assert abs(Ci[k] - Cm[k]) <= 1e-12 * max(1.0, abs(Cm[k])), k
    np.testing.assert_allclose(Ci["dlogits"], Cm["dlogits"], rtol=1e-10, atol=1e-14)
    for name, ref in gm.items():
        np.testing.assert_allclose(gi[name], ref, rtol=1e-10, atol=1e-13, err_msg=name)


def test_gradients_match_central_differences():
    d = O.Dims(D=12, L=2, K=3, hidden=(5,), act="tanh")
    B, S = 3, 4
    p, x, eps = _setup(d, B, S, seed=3)
    _, g = YI.loss_and_grads(d, p, x, eps, S)
    rng = np.random.default_rng(9)
    h = 1e-6
    for name in sorted(p):
        flat = p[name].reshape(-1)
        for i in rng.choice(flat.size, size=min(3, flat.size), replace=False):
            pp = {k: v.copy() for k, v in p.items()}
            pm = {k: v.copy() for k, v in p.items()}
            pp[name].reshape(-1)[i] += h
            pm[name].reshape(-1)[i] -= h
            fd = (YI.loss_and_grads(d, pp, x, eps, S)[0]["loss"] - YI.loss_and_grads(d, pm, x, eps, S)[0]["loss"]) / (2 * h)
            an = g[name].reshape(-1)[i]
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, i, fd, an)


def test_logits_gradient_and_row_weights_closed_form():
    """d loss / d logits = [q (l - sum_k q l) + q (ln q - nent)] / B with the importance-weighted l, and d loss / d log w'_bsk
    = -q_bk softmax_s(log w'_bsk) / B: the row weights rw = q omega the backward epilogues take."""
    d = O.Dims(D=40, L=4, K=6, hidden=(16,))
    B, S = 7, 3
    p, x, eps = _setup(d, B, S, seed=2)
    C0, _ = YI.loss_and_grads(d, p, x, eps, S)
    q, ell = C0["q"], C0["ell"]
    lnq = np.log(q)
    nent = (q * lnq).sum(1, keepdims=True)
    dl = (q * (ell - (q * ell).sum(1, keepdims=True)) + q * (lnq - nent)) / B
    np.testing.assert_allclose(C0["dlogits"], dl, rtol=1e-9, atol=1e-13)
    lw = C0["rows"][:, 3].reshape(B, S, K := d.K)
    om = np.exp(lw - lw.max(axis=1, keepdims=True))
    om /= om.sum(axis=1, keepdims=True)
    # the same weights from the loss as a function of log w' alone
    import torch
    t = torch.tensor(lw, requires_grad=True)
    Lb = (torch.tensor(q) * -(torch.logsumexp(t, dim=1) - np.log(S))).sum(1).mean()
    Lb.backward()
    np.testing.assert_allclose(-t.grad.numpy() * B, q[:, None, :] * om, rtol=1e-12, atol=1e-15)
    assert np.allclose(om.sum(1), 1.0) and K == 6


@pytest.mark.parametrize("S", [1, 2, 7])
def test_bound_sandwich(S):
    d = O.Dims(D=50, L=3, K=5, hidden=(20,))
    B = 9
    for seed in range(3):
        p, x, eps = _setup(d, B, S, seed=10 + seed)
        C0, _ = YI.loss_and_grads(d, p, x, eps, S)
        bound, mlw = YI.enum_bounds(C0, B, S, d.K)
        neg = -C0["per_example"]
        assert (mlw <= neg + 1e-9 * np.abs(neg)).all()
        assert (neg <= bound + 1e-9 * np.abs(bound)).all()
        if S == 1:
            np.testing.assert_allclose(mlw, neg, rtol=1e-12)
        else:
            assert (neg - mlw).max() > 0


def test_header_flag_matches_lib(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    m = re.search(r"GMVAE_OBJ_MARGINAL_Y_IW\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == L.OBJ_MARGINAL_Y_IW == 8
    assert L.OBJ_MARGINAL_Y_IW & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y) == 0
    assert "marginal_iw" in L.Y_INFERENCE and L.lib.gmvae_abi_version() == 7


def _idims(L, B=16, K=10, S=3, flags=None, row0=0, hidden=(64,)):
    return L.make_dims(B, 784, 8, K, hidden, S=S, row0=row0, sched_flags=L.OBJ_MARGINAL_Y_IW if flags is None else flags)


def _ws(L, d, model=None):
    return L.lib.gmvae_workspace_bytes(C.byref(d), L.MODEL_GMVAE if model is None else model, C.byref(C.c_uint64()))


def test_abi_checks(L):
    for model in (L.MODEL_VAE, L.MODEL_VAE_GMP):
        assert _ws(L, _idims(L), model) == -3                                              # GMVAE_E_MODEL
    assert _ws(L, _idims(L)) == 0
    assert _ws(L, _idims(L, S=1)) == 0
    assert _ws(L, _idims(L, flags=L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW, S=1)) == -2       # both objective bits
    assert _ws(L, _idims(L, B=1 << 16, S=1 << 7, K=1 << 8)) == -2                          # B S K = 2^31 > 2^30
    assert _ws(L, _idims(L, B=1 << 16, S=1 << 7, K=1 << 7)) == 0                           # 2^30
    assert _ws(L, _idims(L, B=16, S=2, K=10, row0=1 << 37)) == -2                          # (row0 + B) S K >= 2^38
    assert _ws(L, _idims(L, B=16, S=2, K=10, row0=(1 << 32))) == 0
    # the Gumbel bound refuses the bit; the bound with y summed out ignores it
    assert L.lib.gmvae_iw_bound_workspace_bytes(C.byref(_idims(L)), L.MODEL_GMVAE, C.byref(C.c_uint64())) == -2
    assert L.lib.gmvae_iw_bound(C.byref(_idims(L)), L.MODEL_GMVAE, None, None, 4, None, None, None, None, 0, 0, None) == -2
    b1, b2 = C.c_uint64(), C.c_uint64()
    L.check(L.lib.gmvae_iw_bound_enum_y_workspace_bytes(C.byref(_idims(L)), L.MODEL_GMVAE, C.byref(b1)), "enum ws")
    L.check(L.lib.gmvae_iw_bound_enum_y_workspace_bytes(C.byref(_idims(L, flags=0)), L.MODEL_GMVAE, C.byref(b2)), "enum ws")
    assert b1.value == b2.value


@pytest.mark.parametrize("S,hidden", [(1, (64,)), (3, (64,)), (5, (48, 32))])
def test_workspace_is_the_gumbel_layout_at_s_times_k(L, S, hidden):
    K = 10
    di, dg = _idims(L, S=S, K=K, hidden=hidden), _idims(L, S=S * K, K=K, flags=0, hidden=hidden)
    assert L.workspace_bytes(di, L.MODEL_GMVAE) >= L.workspace_bytes(dg, L.MODEL_GMVAE)
    for name in (b"hg1", b"hd1", b"z", b"logw", b"logq", b"dqp", b"dpp", b"g", b"eps", b"pp", b"y"):
        o1, o2 = C.c_uint64(), C.c_uint64()
        L.check(L.lib.gmvae_workspace_offset(C.byref(di), L.MODEL_GMVAE, name, C.byref(o1)), "offset")
        L.check(L.lib.gmvae_workspace_offset(C.byref(dg), L.MODEL_GMVAE, name, C.byref(o2)), "offset")
        assert o1.value == o2.value, name
    # parameters do not depend on the objective
    assert L.param_layout(di, L.MODEL_GMVAE) == L.param_layout(_idims(L, S=S, flags=0, hidden=hidden), L.MODEL_GMVAE)
    assert L.param_layout(di, L.MODEL_GMVAE) == L.param_layout(_idims(L, S=1, flags=L.OBJ_MARGINAL_Y, hidden=hidden),
                                                               L.MODEL_GMVAE)


def test_schedule_names(L):
    assert L.step_schedule(_idims(L), L.MODEL_GMVAE) == "general+marginal_iw"
    assert L.step_schedule(_idims(L, S=1), L.MODEL_GMVAE) == "general+marginal_iw"
    cfg2 = L.make_dims(1024, 784, 64, 10, (64,), S=2, sched_flags=L.OBJ_MARGINAL_Y_IW)
    assert L.step_schedule(cfg2, L.MODEL_GMVAE).startswith("general+marginal_iw")
    assert L.step_schedule(L.make_dims(1024, 784, 64, 10, (64,), sched_flags=L.OBJ_MARGINAL_Y),
                           L.MODEL_GMVAE).startswith("general+marginal")


def test_factory_rejects_the_vae_family(L):
    from gmvae_amd.engine import Engine
    for model in ("vae", "vae_gmp"):
        with pytest.raises(ValueError, match="marginal_iw"):
            Engine(model, 784, 8, 10, [64], n_samples=3, y_inference="marginal_iw")


def test_runner_flags(L):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    ok = (["--y_inference=marginal_iw"], ["--y_inference=marginal_iw", "--n_samples=5"],
          ["--y_inference=marginal_iw", "--n_samples=3", "--mode=eval", "--iw_enum_samples=50"])
    for args in ok:
        cfg = run_gmvae.check_args(p, p.parse_args(args))
        assert cfg.y_inference == "marginal_iw"
    for bad in (["--y_inference=marginal_iw", "--model=vae"], ["--y_inference=marginal_iw", "--model=vae_gmp"],
                ["--y_inference=marginal_iw", "--iw_samples=10"], ["--y_inference=marginal_iw", "--n_samples=0"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    # the marginal mode's checks are unchanged
    with pytest.raises(SystemExit):
        run_gmvae.check_args(p, p.parse_args(["--y_inference=marginal", "--n_samples=3"]))
