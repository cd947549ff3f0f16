"""gmvae_impute without a device: the fp64 statement (tests/impute_ref.py) against a known answer, the conditions the device
test's cases rest on, and the argument checks of Engine.impute_posterior and the models' impute."""
import math

import numpy as np
import pytest

import impute_cases as IC
import impute_ref as IR
import objective_ref as OR
import oracle as O


# 1 --------------------------------------------------------------------------------------------------------------
def test_statement_against_quadrature():
    """A VAE with one latent dimension, six pixels, three of them missing: p(x_mis | x_obs) and E[x_mis | x_obs] by quadrature
    over z on a fine grid, the statement at n = 4000 within 4 delta-method standard errors computed from its own weights."""
    d = O.Dims(D=6, L=1, K=1, hidden=(8,))
    model = O.MODEL_VAE
    rng = np.random.default_rng(21)
    p = O.init_params(model, d, rng)
    p = {k: v * 3.0 if k.startswith("decoder") else v for k, v in p.items()}      # (a decoder that depends on z visibly)
    x = np.array([[1, 0, 1, 1, 0, 0]], np.uint8)
    m = np.array([[1, 0, 1, 0, 0, 1]], np.uint8)
    obs, mis = m[0] != 0, m[0] == 0
    # the truth: z on a grid, prior N(0, 1), the decoder in fp64
    import torch
    zg = np.linspace(-12.0, 12.0, 480001)
    with torch.no_grad():
        lam = OR._mlp(OR.leaves(p), "decoder", 2, torch.tensor(zg[:, None]), d.act, None, []).numpy() + float(d.gen_bias_init)
    el = x[0][None, :] * lam - np.logaddexp(0.0, lam)                       # log Bernoulli per pixel
    log_joint = -0.5 * zg * zg - 0.5 * math.log(2 * math.pi) + el[:, obs].sum(axis=1)
    w = np.exp(log_joint - log_joint.max())
    w[0] *= 0.5; w[-1] *= 0.5                                               # (trapezoid)
    post = w / w.sum()
    truth_mean = (post[:, None] / (1.0 + np.exp(-lam))).sum(axis=0)
    truth_cond = math.log((post * np.exp(el[:, mis].sum(axis=1))).sum())
    n = 4000
    s = IR.samples(model, d, p, x, m, n, 0, seed=3, step=1)
    e = IR.estimate(s["lw"], s["lam"], s["hid"])
    wn = e["weights"][0]
    sig = 1.0 / (1.0 + np.exp(-s["lam"][0]))
    se_mean = np.sqrt((wn[:, None] ** 2 * (sig - e["mean"][0][None, :]) ** 2).sum(axis=0))
    f = np.exp(s["hid"][0])
    r = (wn * f).sum()
    se_cond = math.sqrt((wn ** 2 * (f - r) ** 2).sum()) / r
    print("mean", e["mean"][0], "truth", truth_mean, "se", se_mean, "cond", e["cond"][0], truth_cond, se_cond, "ess", e["ess"][0])
    assert e["ess"][0] > 100
    assert (np.abs(e["mean"][0] - truth_mean) <= 4 * se_mean).all()
    assert abs(e["cond"][0] - truth_cond) <= 4 * se_cond
    assert abs(math.log(r) - e["cond"][0]) < 1e-12                          # (the two forms of the estimate agree)


# 2 --------------------------------------------------------------------------------------------------------------
def test_cases_hold_their_conditions():
    """Peaked rows and flat rows, weights that are 0 in fp32, few draws too close to compare -- on the statement alone."""
    ess = {name: IC.statement(name, 40)[1]["ess"] for name in IC.CASES}
    assert ess["gumbel-784"].min() < 1.01 and ess["vae-saturated"].min() < 1.01 and ess["vae"].max() > 39.0
    zero_rows = 0
    for name, n, _ in IC.PARAMS:
        s, e = IC.statement(name, n)
        w32 = np.exp((s["lw"] - s["lw"].max(axis=1, keepdims=True)).astype(np.float32))
        zero_rows += int((w32 == 0).any(axis=1).sum())
        left_out = 1.0 - IR.compared_draws(s["lw"], e["key_gap"]).mean()
        assert left_out <= IC.MAX_LEFT_OUT, (name, n, left_out)
        assert np.isfinite(e["mean"]).all() and (e["cond"] <= 0).all()
    assert zero_rows >= 1


def test_fp32_floor_and_gate():
    """The gate of the device test's mean comes from this measurement: the statement in fp32 torch against fp64, on fp32 weights."""
    worst = 0.0
    for name, n, _ in IC.PARAMS:
        model, d, p32 = IC.setup(name)[:3]
        s, _ = IC.statement(name, n)
        lw32 = s["lw"].astype(np.float32).astype(np.float64)
        worst = max(worst, np.abs(IR.mean_fp32(model, d, p32, s["z"], lw32) - IR.estimate(lw32, s["lam"])["mean"]).max())
    print("fp32 floor", worst, "gate", IC.MEAN_GATE)
    assert IC.FP32_FLOOR / 4 <= worst <= 2 * IC.FP32_FLOOR           # (BLAS summation orders differ between hosts)
    assert IC.MEAN_GATE == max(16 * IC.FP32_FLOOR, 1e-6)


def test_weight_bound_is_exact_enough():
    """A self-normalised sum of terms in [0, 1] moves by at most e^{2 g} - 1 when every log weight moves by at most g."""
    rng = np.random.default_rng(0)
    lw, f = rng.normal(0, 30, (200, 17)), rng.random((200, 17))
    for g in (1e-6, 1e-3, 0.3):
        lw2 = lw + rng.uniform(-g, g, lw.shape)
        a = (np.exp(lw - lw.max(1, keepdims=True)) * f).sum(1) / np.exp(lw - lw.max(1, keepdims=True)).sum(1)
        b = (np.exp(lw2 - lw2.max(1, keepdims=True)) * f).sum(1) / np.exp(lw2 - lw2.max(1, keepdims=True)).sum(1)
        assert (np.abs(a - b) <= IR.weight_bound(g)).all()


# 3 --------------------------------------------------------------------------------------------------------------
def test_check_impute_args_refusals():
    from gmvae_amd.engine import check_impute_args
    assert check_impute_args("gmvae", "gumbel", "bernoulli", True, 20, 3, True) == (20, 3)
    assert check_impute_args("vae", "gumbel", "bernoulli", False, 1) == (1, 0)
    for n_draws in (-1, 17):
        with pytest.raises(ValueError, match="n_draws"):
            check_impute_args("gmvae", "gumbel", "bernoulli", True, 20, n_draws)
    with pytest.raises(ValueError, match="n_samples"):
        check_impute_args("gmvae", "gumbel", "bernoulli", True, 0)
    with pytest.raises(ValueError, match="pixel_mask=True"):
        check_impute_args("gmvae", "gumbel", "bernoulli", False, 20, 0, True)
    with pytest.raises(ValueError, match="likelihood"):
        check_impute_args("vae", "gumbel", "gaussian", False, 20)
    for y in ("marginal", "marginal_iw"):
        with pytest.raises(ValueError, match="y_inference"):
            check_impute_args("gmvae", y, "bernoulli", False, 20)
    check_impute_args("vae", "marginal", "bernoulli", False, 20)          # (y_inference means nothing to the VAE family)


def test_model_impute_without_samples_is_base_impute(monkeypatch):
    """model.impute(images, mask) with no further argument returns base.impute's result."""
    from gmvae_amd import base, gmvae, vae
    for cls in (vae.VAE, gmvae.GMVAE):
        obj = object.__new__(cls)
        calls = []
        monkeypatch.setattr(base, "impute", lambda model, images, mask: calls.append((model, images, mask)) or "one-draw")
        monkeypatch.setattr(base, "impute_posterior", lambda *a: pytest.fail("the importance-sampling path"))
        assert obj.impute("images", "mask") == "one-draw" and calls == [(obj, "images", "mask")]
        assert obj.impute("images", "mask", n_samples=None) == "one-draw"
