"""The fp64 statement of gmvae_simulate and gmvae_ais_reverse (tests/bdmc_ref.py) on the CPU: the bidirectional sandwich against
exact quadrature on a two-dimensional latent, the known answer of a decoder that ignores z, the T = 1 identity, the simulation
against the oracle's decoder and the prior's weights, the conditions of every GPU parity case (tests/bdmc_cases.py) -- and every
refusal of the library's host side (no launch, no GPU), the runner's flag and the exported names."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ais_ref as A
import bdmc_cases as K
import bdmc_ref as R
import oracle as O
from oracle.gmvae_oracle import _mlp_fwd

MODELS = K.MODELS


# ---------------------------------------------------------------------------------------------------------------- quadrature
def test_sandwich_against_quadrature():
    """The L = 2 GMVAE of test_ais_cpu (D 24, K 3, hidden 16, tanh), 8 SIMULATED examples, C = 32, 5 leapfrog steps of 0.3: at
    T = 256 every example's upper bound lies within 4 delta-method standard errors of the trapezoid value (and so does the lower
    one); the mean gap upper - lower shrinks from T = 1 to T = 256 and is below 0.15 nats there.
    Measured at these seeds (the first tried): mean gaps 0.522 / 0.162 / 0.069 / 0.057 at T = 1 / 16 / 64 / 256; at T = 256 the worst
    upper bound sits 3.45 and the worst lower bound 2.32 standard errors from the quadrature value."""
    d = O.Dims(D=24, L=2, K=3, hidden=(16,), act="tanh")
    model = O.MODEL_GMVAE
    rng = np.random.default_rng(5)                     # test_ais_cpu.make(model, d, 4, 5)'s parameters
    p = {k: 2.0 * v for k, v in O.init_params(model, d, rng).items()}
    for k in p:
        if k.endswith("/b"):
            p[k] = 0.1 * rng.standard_normal(p[k].shape)
    B, C_ = 8, 32
    rng = np.random.default_rng(23)
    sim = R.simulate(model, d, p, rng.standard_normal((B, 2)), rng.random(B), rng.random((B, d.D)))
    q = A.quadrature_log_px(model, d, p, sim["x"])
    gaps = []
    for T in (1, 16, 64, 256):
        betas = R.schedule("sigmoid", T)
        e, u = rng.standard_normal((T + 1, B * C_, 2)), rng.random((T + 1, B * C_))
        lo = A.ais(model, d, p, sim["x"], betas, C_, 5, 0.3, e, u)
        e, u = rng.standard_normal((T + 1, B * C_, 2)), rng.random((T + 1, B * C_))
        up = R.reverse_ais(model, d, p, sim["x"], sim["z"], betas, C_, 5, 0.3, e, u)
        se_up, se_lo = R.bound_stderr(up["logw"]), R.bound_stderr(lo["logw"])
        gaps.append((up["bound"] - lo["bound"]).mean())
        print(f"T={T}: mean gap {gaps[-1]:.4f}; upper - quad {up['bound'] - q} (worst {np.abs((up['bound'] - q) / se_up).max():.2f} se); "
              f"lower - quad {lo['bound'] - q} (worst {np.abs((lo['bound'] - q) / se_lo).max():.2f} se); reverse accept "
              f"{up['stats'][:, 2].mean():.2f}")
    assert np.all(np.abs(up["bound"] - q) <= 4 * se_up)
    assert np.all(np.abs(lo["bound"] - q) <= 4 * se_lo)
    assert gaps[-1] < gaps[0] and gaps[-1] < 0.15


# ------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("T", [1, 7])
def test_known_answer_of_a_decoder_that_ignores_z(name, T):
    """All decoder weights zero: p(x|z) = p(x), so from the prior base every chain's log w_rev is -log p(x) = -sum_d (x_d lambda_d -
    softplus lambda_d) whatever the chain did, and the upper and the lower bound coincide."""
    model = MODELS[name]
    d = O.Dims(D=23, L=3, K=4, hidden=(16,), act="tanh", gen_bias_init=np.linspace(-0.5, 0.5, 23).astype(np.float32))
    p, _ = K.make(model, d, 3)
    for k in p:
        if k.startswith("decoder") and k.endswith("/w"):
            p[k] = np.zeros_like(p[k])
    rng = np.random.default_rng(4)
    B, C_ = 3, 5
    sim = R.simulate(model, d, p, rng.standard_normal((B, d.L)), rng.random(B), rng.random((B, d.D)))
    betas = R.schedule("sigmoid", T)
    e, u = rng.standard_normal((T + 1, B * C_, d.L)), rng.random((T + 1, B * C_))
    up = R.reverse_ais(model, d, p, sim["x"], sim["z"], betas, C_, 3, 0.5, e, u)
    lo = A.ais(model, d, p, sim["x"], betas, C_, 3, 0.5, e, u)
    lam = _mlp_fwd(p, "decoder", 2, np.zeros((1, d.L)), act=d.act)[0][0] + np.asarray(d.gen_bias_init, np.float64)
    log_px = (sim["x"].astype(np.float64) * lam - O.softplus(lam)).sum(axis=1)
    np.testing.assert_allclose(up["logw"], -np.repeat(log_px[:, None], C_, axis=1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(up["bound"], log_px, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(up["bound"], lo["bound"], rtol=1e-12, atol=1e-12)
    if T > 1:
        assert 0 < up["accepts"].mean()              # the chains moved: the answer does not depend on where to


@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_temperature_from_the_prior_is_minus_the_likelihood_at_z0(name):
    """T = 1, init = "prior": log w_rev = -log p(x | z_0) at the returned z_0."""
    model = MODELS[name]
    d = O.Dims(D=24, L=3, K=4, hidden=(16,), act="relu")
    p, _ = K.make(model, d, 31)
    rng = np.random.default_rng(32)
    B, C_ = 3, 5
    sim = R.simulate(model, d, p, rng.standard_normal((B, d.L)), rng.random(B), rng.random((B, d.D)))
    e, u = rng.standard_normal((2, B * C_, d.L)), rng.random((2, B * C_))
    r = R.reverse_ais(model, d, p, sim["x"], sim["z"], [0.0, 1.0], C_, 3, 0.3, e, u)
    lam, _ = _mlp_fwd(p, "decoder", 2, r["z"], act=d.act)
    xr = np.repeat(sim["x"].astype(np.float64), C_, axis=0)
    np.testing.assert_allclose(r["logw"].reshape(-1), -(xr * lam - O.softplus(lam)).sum(axis=1), rtol=1e-12, atol=1e-12)
    assert r["accepts"].any() and not r["accepts"].all()      # z_0 is the start in some chains and a new point in others


# --------------------------------------------------------------------------------------------------------------- simulation
def test_simulation_against_the_decoder_and_the_cdf():
    model = O.MODEL_VAE_GMP
    d = O.Dims(D=23, L=3, K=4, hidden=(12, 20), act="elu", gen_bias_init=np.linspace(-0.5, 0.5, 23).astype(np.float32))
    p, _ = K.make(model, d, 8)
    lw, mu, sg = R.prior_table(model, d, p)
    cdf = np.cumsum(np.exp(lw))
    # one uniform just below and just above every edge of the CDF, and the two ends
    u = np.concatenate([[0.0], cdf[:-1] - 1e-9, cdf[:-1] + 1e-9, [1.0 - 1e-12]])
    want_k = np.concatenate([[0], np.arange(3), np.arange(1, 4), [3]])
    rng = np.random.default_rng(9)
    B = len(u)
    eps, ux = rng.standard_normal((B, d.L)), rng.random((B, d.D))
    s = R.simulate(model, d, p, eps, u, ux)
    assert np.array_equal(s["k"], want_k)
    np.testing.assert_allclose(s["z"], mu[want_k] + sg[want_k] * eps, rtol=0, atol=0)
    lam, _ = _mlp_fwd(p, "decoder", 3, s["z"], act=d.act)           # the oracle's own decoder
    prob = O.sigmoid(lam + np.asarray(d.gen_bias_init, np.float64))
    assert np.array_equal(s["x"], (ux < prob).astype(np.uint8)) and s["x"].dtype == np.uint8
    np.testing.assert_allclose(s["prob"], prob, rtol=1e-15)
    np.testing.assert_allclose(s["pix_margin"], np.abs(ux - prob), rtol=0, atol=0)
    np.testing.assert_allclose(s["edge"][1:4], 1e-9, rtol=1e-3)
    # one component: no edge
    one = R.simulate(O.MODEL_VAE, d, p, eps, u, ux)
    assert np.all(one["k"] == 0) and np.all(np.isinf(one["edge"])) and np.array_equal(one["z"], eps)


def test_component_frequencies_follow_the_prior():
    """4,000 draws of a K = 4 VAE_GMP: every component's frequency within 4 binomial standard errors of pi_k."""
    model = O.MODEL_VAE_GMP
    d = O.Dims(D=5, L=2, K=4, hidden=(), act="relu")
    p, _ = K.make(model, d, 12)
    rng = np.random.default_rng(13)
    n = 4000
    s = R.simulate(model, d, p, rng.standard_normal((n, d.L)), rng.random(n), rng.random((n, d.D)))
    pi = np.exp(R.prior_table(model, d, p)[0])
    freq = np.bincount(s["k"], minlength=4) / n
    print(f"pi {pi}, frequencies {freq}")
    assert pi.min() > 0.02 and np.all(np.abs(freq - pi) <= 4 * np.sqrt(pi * (1 - pi) / n))


# ---------------------------------------------------------------------------------- the conditions of the GPU parity cases
@pytest.mark.parametrize("case", K.CASES, ids=K.cid)
def test_conditions_of_the_gpu_cases(case):
    """On the statement alone, at the case's own seeds and the CPU restatement of the device's noise: at most 10 % of the chains
    undecided, at most 1 % of the pixels within 1e-5 of their threshold, no component pick within 1e-6 of a CDF edge, and -- for
    a case without explicit T -- an acceptance rate strictly between 0 and 1."""
    model, d, init, B, C_, T, leap, explicit = K.unpack_case(case)
    p, _ = K.case_model(case)
    sim = R.simulate(model, d, p, *K.cpu_sim_noise(B, d))
    z = sim["z"].astype(np.float32).astype(np.float64)       # (the device hands z* on as fp32)
    base = tuple(a.astype(np.float32) for a in A.encoder_table(model, d, p, sim["x"])) if init == "encoder" else None
    eps, u = K.cpu_chain_noise(T, B * C_, d.L)
    r = R.reverse_ais(model, d, p, sim["x"], z, R.schedule("sigmoid", T).astype(np.float32).astype(np.float64), C_, leap, K.STEP0,
                      eps, u, init, base=base)
    und, band, rate = (~r["decided"]).mean(), (sim["pix_margin"] < 1e-5).mean(), r["accepts"].mean()
    print(f"{K.cid(case)}: undecided {und:.3f}, pixels in the band {band:.4f}, nearest CDF edge {sim['edge'].min():.2e}, accept {rate:.2f}")
    assert und <= 0.10 and band <= 0.01 and sim["edge"].min() > 1e-6
    if not explicit:
        assert 0.0 < rate < 1.0


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


E_NULL, E_DIMS, E_MODEL, E_ALIGN = -1, -2, -3, -4


def _dims(lib_, **kw):
    return lib_.make_dims(kw.pop("B", 4), kw.pop("D", 784), kw.pop("L", 64), kw.pop("K", 10), kw.pop("hidden", [64]), **kw)


def _rev(L, cd, model=2, x=256, params=256, base=None, base_K=0, z_start=256, betas=256, T=8, C_=16, leap=3, step0=0.5, up=1.02,
         down=0.96, tail=256, ws=256, z_out=None):
    """gmvae_ais_reverse on made-up addresses: every refusal comes back before any launch, so nothing is dereferenced."""
    return L.lib.gmvae_ais_reverse(C.byref(cd) if cd is not None else None, model, x, params, base, base_K, z_start, betas, T, C_,
                                   leap, step0, up, down, None, None, None, None, None, z_out, tail, ws, 0, 0, None)


def _sim(L, cd, model=2, params=256, eps=None, u=None, ux=None, z=256, k=256, x=256, prob=None, ws=256):
    return L.lib.gmvae_simulate(C.byref(cd) if cd is not None else None, model, params, eps, u, ux, z, k, x, prob, ws, 0, 0, None)


def test_refusals_of_the_reverse_chains(L):
    ok = lambda **kw: _dims(L, **kw)
    assert _rev(L, None) == E_NULL
    assert _rev(L, ok(), model=3) == E_MODEL
    for bad in (dict(hidden=[64, 64, 64, 64]), dict(hidden=[513]), dict(L=129), dict(L=0), dict(K=65), dict(D=0), dict(B=0)):
        assert _rev(L, ok(**bad)) == E_DIMS, bad
    assert _rev(L, ok(), base=256, base_K=65) == E_DIMS
    for flag in (L.LIK_GREY_BERNOULLI, L.LIK_CONT_BERNOULLI, L.LIK_GAUSSIAN, L.OBJ_PIXEL_MASK, L.LIK_GAUSSIAN | L.X_F32,
                 L.LIK_GAUSSIAN | L.LIK_SCALE_LEARNED):
        assert _rev(L, ok(sched_flags=flag)) == E_DIMS
    assert _rev(L, ok(), T=0) == E_DIMS and _rev(L, ok(), C_=0) == E_DIMS and _rev(L, ok(), leap=0) == E_DIMS
    assert _rev(L, ok(row0=(1 << 38) // 16 - 4), C_=16) == E_DIMS
    assert _rev(L, ok(row0=(1 << 38) // 16 - 5), C_=16, x=None) == E_NULL
    assert _rev(L, ok(), step0=0.0) == E_DIMS and _rev(L, ok(), up=float("nan")) == E_DIMS and _rev(L, ok(), down=float("inf")) == E_DIMS
    # the sizes come before the pointers, the pointers before the alignment
    assert _rev(L, ok(L=129), z_start=None) == E_DIMS
    for missing in ("x", "params", "betas", "tail", "ws", "z_start"):
        assert _rev(L, ok(), **{missing: None}) == E_NULL, missing
    assert _rev(L, ok(), base=None, base_K=1) == E_NULL and _rev(L, ok(), base=256, base_K=0) == E_DIMS
    assert _rev(L, ok(), z_start=None, params=260) == E_NULL
    for odd in (dict(params=260), dict(ws=128), dict(betas=258), dict(z_start=258), dict(z_out=258)):
        assert _rev(L, ok(), **odd) == E_ALIGN, odd
    # the size query: gmvae_ais's gates and gmvae_ais's layout
    b = C.c_uint64()
    q = lambda cd, model=2, bk=0, c=16: L.lib.gmvae_ais_reverse_workspace_bytes(C.byref(cd), model, bk, c, C.byref(b))
    assert q(ok(hidden=[513])) == E_DIMS and q(ok(L=129)) == E_DIMS and q(ok(K=65)) == E_DIMS and q(ok(), c=0) == E_DIMS
    assert q(ok(sched_flags=L.OBJ_PIXEL_MASK)) == E_DIMS
    assert q(ok(D=3073, L=128, K=64, hidden=[512, 512, 512]), bk=64) == 0 and b.value > 0
    assert L.lib.gmvae_ais_reverse_workspace_bytes(C.byref(ok()), 2, 0, 16, None) == E_NULL
    assert L.ais_reverse_workspace_bytes(ok(B=8), 2, 10, 16) == L.ais_workspace_bytes(ok(B=8), 2, 10, 16)


def test_refusals_of_the_simulation(L):
    ok = lambda **kw: _dims(L, **kw)
    assert _sim(L, None) == E_NULL
    assert _sim(L, ok(), model=-1) == E_MODEL
    for bad in (dict(hidden=[64, 64, 64, 64]), dict(hidden=[513]), dict(hidden=[64, 0]), dict(L=129), dict(K=65), dict(D=0), dict(B=0)):
        assert _sim(L, ok(**bad)) == E_DIMS, bad
    assert _sim(L, ok(K=65), model=0, params=None) == E_NULL      # (the VAE's prior has one component whatever K says)
    for flag in (L.LIK_GREY_BERNOULLI, L.LIK_CONT_BERNOULLI, L.LIK_GAUSSIAN, L.OBJ_PIXEL_MASK, L.LIK_GAUSSIAN | L.X_F32):
        assert _sim(L, ok(sched_flags=flag)) == E_DIMS
    assert _sim(L, ok(row0=(1 << 38) - 4)) == E_DIMS               # row0 + B = 2^38
    assert _sim(L, ok(row0=(1 << 38) - 5), params=None) == E_NULL  # ... one row less passes the sizes
    assert _sim(L, ok(L=129), params=None) == E_DIMS
    for missing in ("params", "z", "k", "x", "ws"):
        assert _sim(L, ok(), **{missing: None}) == E_NULL, missing
    assert _sim(L, ok(), z=None, params=260) == E_NULL
    for odd in (dict(params=260), dict(ws=128), dict(eps=258), dict(u=258), dict(ux=258), dict(z=258), dict(k=258), dict(x=258),
                dict(prob=258)):
        assert _sim(L, ok(), **odd) == E_ALIGN, odd
    b = C.c_uint64()
    q = lambda cd, model=2: L.lib.gmvae_simulate_workspace_bytes(C.byref(cd), model, C.byref(b))
    assert q(ok(hidden=[513])) == E_DIMS and q(ok(L=129)) == E_DIMS and q(ok(K=65)) == E_DIMS and q(ok(), model=3) == E_MODEL
    assert q(ok(sched_flags=L.OBJ_PIXEL_MASK)) == E_DIMS
    assert L.lib.gmvae_simulate_workspace_bytes(C.byref(ok()), 2, None) == E_NULL
    n = L.simulate_workspace_bytes(ok(B=8), 2)
    assert n == L.simulate_workspace_bytes(ok(B=4096, D=50000), 2) and 0 < n < 10 * 64 * 4 * 2 + 4096      # the prior table alone


# ------------------------------------------------------------------------------------------------------- flags and names
def test_runner_flags():
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    cfg = p.parse_args(["--mode=eval", "--ais_chains=8", "--ais_temps=100", "--bdmc_examples=64"])
    run_gmvae.check_args(p, cfg)
    assert cfg.bdmc_examples == 64 and p.parse_args([]).bdmc_examples == 0
    for bad in (["--mode=eval", "--bdmc_examples=8"], ["--mode=eval", "--bdmc_examples=8", "--ais_chains=8"],
                ["--bdmc_examples=8", "--ais_chains=8", "--ais_temps=8"],
                ["--mode=eval", "--bdmc_examples=-1", "--ais_chains=8", "--ais_temps=8"],
                ["--mode=eval", "--bdmc_examples=8", "--ais_chains=8", "--ais_temps=8", "--missing_rate=0.5"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))


def test_the_new_names_are_declared_and_bound(L):
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gmvae_hip.h")).read()
    for name in ("gmvae_simulate_workspace_bytes", "gmvae_simulate", "gmvae_ais_reverse_workspace_bytes", "gmvae_ais_reverse"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in L.EXPORTS and hasattr(L.lib, name)
    assert L.lib.gmvae_abi_version() == 7
