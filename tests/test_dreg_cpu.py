"""CPU side of the doubly reparameterised gradient (include/gmvae_hip.h GMVAE_GRAD_DREG): the flag, the workspace size, the
refusals and the schedule names of the C ABI, the Engine / factory / runner arguments, and the fp64 statement itself
(tests/dreg_ref.py): generative gradients equal to the standard statement's, the closed form at S = 1, and unbiasedness
against the plain reparameterised estimator over 20,000 noise draws."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dreg_ref as DR
import oracle as O
import ymarg_iw_ref as YI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"vae": O.MODEL_VAE, "vae_gmp": O.MODEL_VAE_GMP, "gmvae": O.MODEL_GMVAE}


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the library
def test_flag_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    m = re.search(r"GMVAE_GRAD_DREG\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == L.GRAD_DREG == 16
    assert L.GRAD_DREG & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW) == 0
    assert L.GRAD_ESTIMATORS == ("standard", "dreg")
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


WS_DIMS = [   # (model, B, D, Lz, K, hidden, S, objective flags)
    ("vae", 1024, 784, 2, 1, (64,), 1, 0),                 # configs[0]: a one-launch schedule without the bit
    ("vae", 64, 784, 2, 1, (64,), 5, 0),
    ("vae_gmp", 256, 784, 64, 10, (64,), 50, 0),
    ("vae_gmp", 32, 784, 64, 10, (64,), 1, 0),
    ("vae", 32, 784, 32, 1, (512,), 1, 0),                 # skinny without the bit
    ("gmvae", 1024, 784, 64, 10, (64,), 1, 4),             # marginal
    ("gmvae", 1024, 784, 64, 10, (64,), 1, 8),             # marginal_iw at S = 1: ymarg_rows, no v
    ("gmvae", 1024, 784, 64, 10, (64,), 5, 8),
    ("gmvae", 5, 96, 6, 6, (16,), 3, 8),
    ("gmvae", 24, 200, 16, 7, (64, 64), 70, 8),
]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"{c[0]}-B{c[1]}-L{c[3]}-S{c[6]}-f{c[7]}")
def test_workspace_bytes(L, case):
    """Without the bit the size is what it is at bit 0 of this build whatever the other bits; the bit adds bytes only under
    GMVAE_OBJ_MARGINAL_Y_IW at S > 1: the [B*S*K] floats of v, rounded to 256 bytes, behind every other buffer."""
    name, B, D, Lz, K, hidden, S, obj = case
    model = L.MODEL_IDS[name]
    base = L.workspace_bytes(L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=obj), model)
    assert base == L.workspace_bytes(L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=obj | L.SCHED_SAFE), model)
    with_bit = L.workspace_bytes(L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=obj | L.GRAD_DREG), model)
    if obj == L.OBJ_MARGINAL_Y_IW and S > 1:
        assert with_bit - base == (B * S * K * 4 + 255) // 256 * 256
    else:
        assert with_bit == base
    # no existing offset moves with the bit
    for buf in (b"z", b"dqp", b"slabs", b"logw", b"dlogits" if name == "gmvae" else b"qp"):
        o0, o1 = C.c_uint64(), C.c_uint64()
        L.check(L.lib.gmvae_workspace_offset(C.byref(L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=obj)), model, buf,
                                             C.byref(o0)), "offset")
        L.check(L.lib.gmvae_workspace_offset(C.byref(L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=obj | L.GRAD_DREG)), model,
                                             buf, C.byref(o1)), "offset")
        assert o0.value == o1.value, buf


def test_gumbel_gmvae_is_refused(L):
    for S in (1, 3):
        d = L.make_dims(16, 784, 8, 10, (64,), S=S, sched_flags=L.GRAD_DREG)
        assert L.lib.gmvae_workspace_bytes(C.byref(d), L.MODEL_GMVAE, C.byref(C.c_uint64())) == -2
        assert L.lib.gmvae_step(C.byref(d), L.MODEL_GMVAE, None, None, None, None, None, None, 0, 0, None, None) == -2
        assert L.lib.gmvae_step_schedule(C.byref(d), L.MODEL_GMVAE, C.create_string_buffer(48)) == -2
        # the same dims are fine for the VAE family and with an objective bit
        for model in (L.MODEL_VAE, L.MODEL_VAE_GMP):
            assert L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(C.c_uint64())) == 0
            assert L.lib.gmvae_step(C.byref(d), model, None, None, None, None, None, None, 0, 0, None, None) == -1      # (NULL, not DIMS)
        d.sched_flags = L.GRAD_DREG | L.OBJ_MARGINAL_Y_IW
        assert L.lib.gmvae_workspace_bytes(C.byref(d), L.MODEL_GMVAE, C.byref(C.c_uint64())) == 0
    d = L.make_dims(16, 784, 8, 10, (64,), S=1, sched_flags=L.GRAD_DREG | L.OBJ_MARGINAL_Y)
    assert L.lib.gmvae_workspace_bytes(C.byref(d), L.MODEL_GMVAE, C.byref(C.c_uint64())) == 0


def test_bounds_and_posteriors_mask_the_bit(L):
    """gmvae_iw_bound* / gmvae_posterior_*: the same workspace with and without the bit, the Gumbel GMVAE included."""
    fns = ((L.iw_bound_workspace_bytes, (L.MODEL_VAE, L.MODEL_VAE_GMP, L.MODEL_GMVAE)),
           (L.iw_bound_enum_y_workspace_bytes, (L.MODEL_GMVAE,)), (L.posterior_y_workspace_bytes, (L.MODEL_GMVAE,)),
           (L.posterior_component_workspace_bytes, (L.MODEL_VAE_GMP,)))
    for fn, models in fns:
        for model in models:
            a = fn(L.make_dims(16, 784, 8, 10, (64,), S=5), model)
            assert a == fn(L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=L.GRAD_DREG), model)
    a = L.iw_bound_enum_y_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5), L.MODEL_GMVAE)
    assert a == L.iw_bound_enum_y_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5,
                                                              sched_flags=L.GRAD_DREG | L.OBJ_MARGINAL_Y_IW), L.MODEL_GMVAE)


def test_schedule_names(L):
    cfg2 = dict(B=1024, D=784, L=64, K=10, hidden=(64,))
    assert L.step_schedule(L.make_dims(S=5, sched_flags=L.GRAD_DREG | L.OBJ_MARGINAL_Y_IW, **cfg2),
                           L.MODEL_GMVAE) == "general+marginal_iw+dreg"
    assert L.step_schedule(L.make_dims(S=1, sched_flags=L.GRAD_DREG | L.OBJ_MARGINAL_Y, **cfg2),
                           L.MODEL_GMVAE) == "general+marginal+dreg"
    cfg0 = dict(B=1024, D=784, L=2, K=1, hidden=(64,))
    assert L.step_schedule(L.make_dims(**cfg0), L.MODEL_VAE).startswith("mega")
    assert L.step_schedule(L.make_dims(sched_flags=L.GRAD_DREG, **cfg0), L.MODEL_VAE) == "general+dreg"
    cfg1 = dict(B=256, D=784, L=64, K=10, hidden=(64,))
    assert L.step_schedule(L.make_dims(**cfg1), L.MODEL_VAE_GMP).startswith("mega")
    assert L.step_schedule(L.make_dims(sched_flags=L.GRAD_DREG, **cfg1), L.MODEL_VAE_GMP) == "general+dreg"
    wide = dict(B=32, D=784, L=32, K=1, hidden=(512,))
    assert L.step_schedule(L.make_dims(**wide), L.MODEL_VAE) == "skinny"
    assert L.step_schedule(L.make_dims(sched_flags=L.GRAD_DREG, **wide), L.MODEL_VAE) == "general+dreg"
    # without the bit nothing is renamed
    assert L.step_schedule(L.make_dims(S=5, sched_flags=L.OBJ_MARGINAL_Y_IW, **cfg2), L.MODEL_GMVAE) == "general+marginal_iw"


def test_engine_and_factory_arguments(L):
    from gmvae_amd import gmvae, vae
    from gmvae_amd.engine import Engine
    with pytest.raises(ValueError, match="grad_estimator"):
        Engine("vae", 784, 8, 1, [64], grad_estimator="sticking")
    for kw in (dict(), dict(n_samples=3)):
        with pytest.raises(ValueError, match="marginal.*marginal_iw"):
            Engine("gmvae", 784, 8, 10, [64], grad_estimator="dreg", **kw)
        with pytest.raises(ValueError, match="marginal.*marginal_iw"):
            gmvae.create_gmvae(784, 8, mixture_components=10, fcnet_hidden_sizes=[64], grad_estimator="dreg", **kw)
    with pytest.raises(ValueError, match="grad_estimator"):
        vae.create_vae(784, 8, fcnet_hidden_sizes=[64], grad_estimator="nope")


def test_runner_flags(L):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    assert p.parse_args([]).grad_estimator == "standard"
    d = p.parse_args([])
    assert (d.y_inference, d.n_samples, d.model, d.latent_size, d.batch_size) == ("gumbel", 1, "gmvae", 8, 16)
    ok = (["--grad_estimator=dreg", "--model=vae"], ["--grad_estimator=dreg", "--model=vae_gmp", "--n_samples=5"],
          ["--grad_estimator=dreg", "--y_inference=marginal"],
          ["--grad_estimator", "dreg", "--y_inference=marginal_iw", "--n_samples", "3"])
    for args in ok:
        assert run_gmvae.check_args(p, p.parse_args(args)).grad_estimator == "dreg"
    assert run_gmvae.check_args(p, p.parse_args(["--grad_estimator=standard"])).grad_estimator == "standard"
    for bad in (["--grad_estimator=dreg"], ["--grad_estimator=dreg", "--model=gmvae", "--n_samples=3"], ["--grad_estimator=stl"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))


# ---------------------------------------------------------------------------------------- the fp64 statement
def _setup(model, d, B, S, seed=0):
    p = O.init_params(model, d, np.random.default_rng(seed))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.1, p[k].shape)
    x, _, _ = O.make_inputs(d, B, model, seed_x=100 + seed)
    rows = B * S * (d.K if model == O.MODEL_GMVAE else 1)
    eps = np.random.default_rng(seed + 1).standard_normal((rows, d.L))
    return p, x, eps


CASES = [("vae", O.Dims(D=30, L=3, K=1, hidden=(12,)), 5, 1), ("vae", O.Dims(D=30, L=3, K=1, hidden=(12, 9), act="tanh"), 5, 4),
         ("vae_gmp", O.Dims(D=30, L=4, K=5, hidden=(12,)), 4, 3), ("vae_gmp", O.Dims(D=30, L=4, K=5, hidden=(12,)), 4, 1),
         ("gmvae", O.Dims(D=30, L=3, K=4, hidden=(12, 9)), 5, 1), ("gmvae", O.Dims(D=30, L=3, K=4, hidden=(12,), sigma_min=0.9), 3, 4)]


@pytest.mark.parametrize("name,d,B,S", CASES, ids=[f"{c[0]}-S{c[3]}" for c in CASES])
def test_generative_gradients_are_the_standard_statements(name, d, B, S):
    """Loss, terms, dlogits and every non-inference gradient of the DReG statement equal the standard reference's (the
    oracle's closed form for the VAE family, tests/ymarg_iw_ref.py for the GMVAE) to 1e-12; the inference gradient differs."""
    model = MODELS[name]
    p, x, eps = _setup(model, d, B, S, seed=len(name) + S)
    Cd, gd = DR.loss_and_grads(model, d, p, x, eps, S)
    Cs, gs = DR.loss_and_grads(model, d, p, x, eps, S, estimator="standard")
    if model == O.MODEL_GMVAE:
        Cr, gr = YI.loss_and_grads(d, p, x, eps, S)
        np.testing.assert_allclose(Cd["dlogits"], Cr["dlogits"], rtol=1e-12, atol=1e-15)
    else:
        import dataclasses
        Cr, gr = O.loss_and_grads(model, dataclasses.replace(d, S=S), p, x, eps, None, np.float64)
    for k in ("loss", "nll", "kl", "nent"):
        assert abs(Cd[k] - Cr[k]) <= 1e-12 * max(1.0, abs(Cr[k])), k
    moved = 0.0
    for k, ref in gr.items():
        scale = max(np.abs(ref).max(), 1e-30)
        assert np.abs(gs[k] - ref).max() <= 1e-12 * max(scale, 1.0), k           # the statement's standard estimator is the reference
        if DR.is_inference(model, k):
            moved = max(moved, np.abs(gd[k] - ref).max() / scale)
        else:
            assert np.abs(gd[k] - ref).max() <= 1e-12 * max(scale, 1.0), k
    assert moved > 1e-3


@pytest.mark.parametrize("name,d,B,S", CASES, ids=[f"{c[0]}-S{c[3]}" for c in CASES])
def test_seeds_at_z_are_the_closed_form(name, d, B, S):
    """dmu_q = v (dz + w pterm - w eps / sig_q), dsig_q = dmu_q eps against the standard dmu_q = dz + w pterm, dsig_q = dmu_q eps
    - w / sig_q on the same inputs (dz + w pterm is the standard dmu_q); at S = 1 v = 1."""
    model = MODELS[name]
    p, x, eps = _setup(model, d, B, S, seed=3 + S)
    Cd, _ = DR.loss_and_grads(model, d, p, x, eps, S)
    Cs, _ = DR.loss_and_grads(model, d, p, x, eps, S, estimator="standard")
    w, v, sig = Cs["w"][:, None], Cs["v"][:, None], Cs["sig_q"]
    if S == 1:
        assert np.array_equal(Cs["v"], np.ones_like(Cs["v"]))
    dmu = v * (Cs["dmu"] - w * eps / sig)
    np.testing.assert_allclose(Cd["dmu"], dmu, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(Cd["dsig"], dmu * eps, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(Cs["dsig"], Cs["dmu"] * eps - w / sig, rtol=1e-10, atol=1e-13)


def test_unbiased_against_the_reparameterised_estimator():
    """VAE D = 16, L = 3, hidden (8,), B = 2, S = 4: the encoder gradient averaged over N = 20,000 noise draws under both
    estimators agrees within 4 standard errors of the (paired) difference on every coordinate.  The N draws run as one batch of
    N copies of the two examples; a draw's encoder gradient is J^T (its gradient at the encoder's output), J = the encoder's
    Jacobian, which does not depend on the noise."""
    import torch
    d = O.Dims(D=16, L=3, K=1, hidden=(8,))
    B, S, N = 2, 4, 20000
    model = O.MODEL_VAE
    p = O.init_params(model, d, np.random.default_rng(11))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(12).normal(0, 0.1, p[k].shape)
    x = (np.random.default_rng(13).random((B, d.D)) < 0.6).astype(np.uint8)
    eps = np.random.default_rng(14).standard_normal((N * B * S, d.L))
    xs = np.tile(x, (N, 1))
    Cd, gd = DR.loss_and_grads(model, d, p, xs, eps, S)
    Cs, gs = DR.loss_and_grads(model, d, p, xs, eps, S, estimator="standard")
    names = [k for k in sorted(p) if DR.is_inference(model, k)]
    t = {k: torch.tensor(p[k], requires_grad=True) for k in names}
    h = torch.relu(torch.tensor(x, dtype=torch.float64) @ t["encoder_fcnet/linear_0/w"] + t["encoder_fcnet/linear_0/b"])
    out = (h @ t["encoder_fcnet/linear_1/w"] + t["encoder_fcnet/linear_1/b"]).reshape(-1)               # [B * 2L]
    J = torch.stack([torch.cat([g.reshape(-1) for g in torch.autograd.grad(out[i], [t[k] for k in names], retain_graph=True)])
                     for i in range(out.numel())]).numpy()                                              # [B*2L, P_enc]
    per_draw = {}
    for tag, Cc, g in (("dreg", Cd, gd), ("standard", Cs, gs)):
        gn = Cc["dqp"].reshape(N, B * 2 * d.L) @ J                                                       # [N, P_enc]: B * loss per draw
        whole = np.concatenate([g[k].reshape(-1) for k in names]) * (N * B)
        np.testing.assert_allclose(gn.sum(axis=0), whole, rtol=1e-9, atol=1e-9)      # the draws add up to the statement's gradient
        per_draw[tag] = gn
    diff = per_draw["dreg"] - per_draw["standard"]
    se = diff.std(axis=0, ddof=1) / np.sqrt(N)
    ok = se > 0
    assert ok.sum() >= 50                      # (the rest: weights of zero pixels and of units whose ReLU is off for both examples)
    zscore = np.abs(diff.mean(axis=0)[ok]) / se[ok]
    print(f"unbiasedness: {int(ok.sum())} coordinates, max |z| {zscore.max():.2f}, mean |z| {zscore.mean():.2f}")
    assert zscore.max() <= 4.0, (zscore.max(), int(zscore.argmax()))
    # and the two are different estimators: per draw they differ by far more than rounding
    assert np.abs(diff).max() > 1e-3 * np.abs(per_draw["standard"]).max()
