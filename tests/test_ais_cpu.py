"""The fp64 statement of gmvae_ais (tests/ais_ref.py) on the CPU: against exact quadrature on a two-dimensional latent, its
gradients against torch.autograd, the T = 1 identities against oracle.forward, the schedule -- and every refusal of the library's
host side (no launch, no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ais_ref as R
import oracle as O

MODELS = {"vae": O.MODEL_VAE, "vae_gmp": O.MODEL_VAE_GMP, "gmvae": O.MODEL_GMVAE}


def make(model, d, B, seed, scale=2.0):
    rng = np.random.default_rng(seed)
    p = {k: scale * v for k, v in O.init_params(model, d, rng).items()}
    for k in p:
        if k.endswith("/b"):
            p[k] = 0.1 * rng.standard_normal(p[k].shape)
    x = (rng.random((B, d.D)) < 0.5).astype(np.uint8)
    return p, x, rng


# ---------------------------------------------------------------------------------------------------------------- quadrature
QUAD_D = O.Dims(D=24, L=2, K=3, hidden=(16,), act="tanh")
_QUAD = {}


def quad_case():
    """(params, x, quadrature log p(x)) of the L = 2 GMVAE, computed once."""
    if not _QUAD:
        p, x, _ = make(O.MODEL_GMVAE, QUAD_D, 4, 5)
        _QUAD["v"] = (p, x, R.quadrature_log_px(O.MODEL_GMVAE, QUAD_D, p, x))
    return _QUAD["v"]


def test_statement_against_quadrature():
    """At T = 256, C = 64, 5 leapfrog steps of 0.3 every example's bound lies within 4 delta-method standard errors of the
    trapezoid value on an 801 x 801 grid over [-8, 8]^2; at T = 1, 16, 64, 256 the mean absolute error does not grow."""
    p, x, q = quad_case()
    rng = np.random.default_rng(11)
    C_, errs = 64, []
    for T in (1, 16, 64, 256):
        e, u = rng.standard_normal((T + 1, 4 * C_, 2)), rng.random((T + 1, 4 * C_))
        r = R.ais(O.MODEL_GMVAE, QUAD_D, p, x, R.schedule("sigmoid", T), C_, 5, 0.3, e, u)
        errs.append(np.abs(r["bound"] - q).mean())
        se = R.bound_stderr(r["logw"])
        print(f"T={T}: err {r['bound'] - q}, se {se}, accept {r['stats'][:, 2]}")
    assert np.all(np.abs(r["bound"] - q) <= 4 * se)
    assert errs[-1] < errs[0] and errs[-1] < 0.1


# ------------------------------------------------------------------------------------------------------------------ gradient
def _torch_parts(model, d, p, x, C_, z, base):
    """(A, B) of the statement for init="encoder" written with torch in fp64: log r(z), log p(z) + log p(x|z)."""
    tp = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}
    act = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "elu": torch.nn.functional.elu}[d.act]

    def mix(lw, mu, sg):
        lw, mu, sg = (torch.tensor(np.asarray(a, np.float64)) for a in (lw, mu, sg))
        if lw.ndim == 1:
            lw, mu, sg = lw[None], mu[None], sg[None]
        n = torch.distributions.Normal(mu, sg).log_prob(z[:, None, :]).sum(dim=2)
        return torch.logsumexp(lw + n, dim=1)

    h = z
    nl = len(d.hidden) + 1
    for i in range(nl):
        h = h @ tp[f"decoder_fcnet/linear_{i}/w"] + tp[f"decoder_fcnet/linear_{i}/b"]
        if i < nl - 1:
            h = act(h)
    lam = h + torch.tensor(np.asarray(d.gen_bias_init, np.float64))
    xr = torch.tensor(np.repeat(np.asarray(x).astype(np.float64), C_, axis=0))
    logpx = (xr * lam - torch.nn.functional.softplus(lam)).sum(dim=1)
    lw, mu, sg = base
    rep = lambda a: np.repeat(np.asarray(a), C_, axis=0)
    return mix(rep(lw), rep(mu), rep(sg)), mix(*R.prior_table(model, d, p)) + logpx


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("act,hidden", [("relu", (12, 20)), ("tanh", (16,)), ("elu", ())])
def test_gradient_against_autograd(name, act, hidden):
    model = MODELS[name]
    d = O.Dims(D=23, L=5, K=4, hidden=hidden, act=act, gen_bias_init=np.linspace(-1, 1, 23))
    p, x, rng = make(model, d, 3, 21)
    C_ = 4
    base = R.encoder_table(model, d, p, x)
    tg = R.Target(model, d, p, x, C_, "encoder", base)
    zn = rng.standard_normal((3 * C_, d.L))
    vA, vB, gA, gB, _ = tg.parts(zn)
    z = torch.tensor(zn, requires_grad=True)
    tA, tB = _torch_parts(model, d, p, x, C_, z, base)
    tgA, = torch.autograd.grad(tA.sum(), z, retain_graph=True)
    tgB, = torch.autograd.grad(tB.sum(), z)
    np.testing.assert_allclose(vA, tA.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(vB, tB.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gA, tgA.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(gB, tgB.numpy(), rtol=1e-10, atol=1e-10)
    # the prior as the base: A = log p(z), B = log p(x|z): the same sum, split differently
    pA, pB, pgA, pgB, _ = R.Target(model, d, p, x, C_, "prior").parts(zn)
    np.testing.assert_allclose(pA + pB, vB, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(pgA + pgB, gB, rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_temperature_from_the_prior_is_the_likelihood_at_z0(name):
    """T = 1, init="prior": log w = log p(x|z_0), z_0 the prior's draw."""
    model = MODELS[name]
    d = O.Dims(D=24, L=3, K=4, hidden=(16,), act="relu")
    p, x, rng = make(model, d, 3, 31)
    C_ = 5
    e, u = rng.standard_normal((2, 3 * C_, d.L)), rng.random((2, 3 * C_))
    r = R.ais(model, d, p, x, [0.0, 1.0], C_, 3, 0.5, e, u, init="prior")
    tg = R.Target(model, d, p, x, C_, "prior")
    z0, _ = tg.start(e[0], u[0])
    lam, _ = O.gmvae_oracle._mlp_fwd({k: np.asarray(v, np.float64) for k, v in p.items()}, "decoder", 2, z0, act=d.act)
    xr = np.repeat(x.astype(np.float64), C_, axis=0)
    want = (xr * lam - O.softplus(lam)).sum(axis=1)
    np.testing.assert_allclose(r["logw"].reshape(-1), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["vae", "vae_gmp"])
def test_one_temperature_from_the_encoder_is_the_forward_log_weight(name):
    """T = 1, init="encoder": log w is oracle.forward's logw at S = C on the same eps."""
    model = MODELS[name]
    C_ = 6
    d = O.Dims(D=24, L=3, K=4, hidden=(16,), act="relu", S=C_)
    p, x, rng = make(model, d, 3, 41)
    e, u = rng.standard_normal((2, 3 * C_, d.L)), rng.random((2, 3 * C_))
    r = R.ais(model, d, p, x, [0.0, 1.0], C_, 3, 0.5, e, u, init="encoder")
    f = O.forward(model, d, p, x, e[0])
    np.testing.assert_allclose(r["logw"].reshape(-1), f["logw"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(r["bound"], f["bound"], rtol=1e-11, atol=1e-11)


def test_schedules():
    for kind in ("linear", "sigmoid"):
        for T in (1, 2, 8, 1000):
            b = R.schedule(kind, T)
            assert b[0] == 0.0 and b[-1] == 1.0 and len(b) == T + 1 and np.all(np.diff(b) > 0)
    s = lambda v: 1.0 / (1.0 + math.exp(-v))
    assert R.schedule("sigmoid", 4)[1] == pytest.approx((s(-2.0) - s(-4.0)) / (s(4.0) - s(-4.0)), rel=1e-14)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def _call(L, cd, model=2, x=256, params=256, base=None, base_K=0, betas=256, T=8, C_=16, leap=3, step0=0.5, up=1.02, down=0.96,
          tail=256, ws=256):
    """gmvae_ais on made-up addresses: every refusal comes back before any launch, so nothing is dereferenced."""
    return L.lib.gmvae_ais(C.byref(cd) if cd is not None else None, model, x, params, base, base_K, betas, T, C_, leap, step0, up,
                           down, None, None, None, None, None, None, tail, ws, 0, 0, None)


def test_refusals(L):
    E_NULL, E_DIMS, E_MODEL, E_ALIGN = -1, -2, -3, -4
    ok = lambda **kw: L.make_dims(kw.pop("B", 4), kw.pop("D", 784), kw.pop("L", 64), kw.pop("K", 10), kw.pop("hidden", [64]), **kw)
    # the sizes
    assert _call(L, None) == E_NULL
    assert _call(L, ok(), model=3) == E_MODEL
    assert _call(L, ok(hidden=[64, 64, 64, 64])) == E_DIMS
    assert _call(L, ok(hidden=[513])) == E_DIMS
    assert _call(L, ok(hidden=[64, 0])) == E_DIMS
    assert _call(L, ok(L=129)) == E_DIMS
    assert _call(L, ok(L=0)) == E_DIMS
    assert _call(L, ok(K=65)) == E_DIMS
    assert _call(L, ok(K=65), model=0, x=None) == E_NULL      # (the VAE's prior has one component whatever K says)
    assert _call(L, ok(D=0)) == E_DIMS
    assert _call(L, ok(B=0)) == E_DIMS
    assert _call(L, ok(), base=256, base_K=65) == E_DIMS
    # the likelihoods and the mask
    for flag in (L.LIK_GREY_BERNOULLI, L.LIK_CONT_BERNOULLI, L.LIK_GAUSSIAN, L.OBJ_PIXEL_MASK, L.LIK_GAUSSIAN | L.X_F32,
                 L.LIK_GAUSSIAN | L.LIK_SCALE_LEARNED):
        assert _call(L, ok(sched_flags=flag)) == E_DIMS
    # the counts
    assert _call(L, ok(), T=0) == E_DIMS
    assert _call(L, ok(), C_=0) == E_DIMS
    assert _call(L, ok(), leap=0) == E_DIMS
    assert _call(L, ok(row0=(1 << 38) // 16 - 4), C_=16) == E_DIMS          # (row0 + B) C = 2^38
    assert _call(L, ok(row0=(1 << 38) // 16 - 5), C_=16, x=None) == E_NULL  # ... one row less passes the sizes
    assert _call(L, ok(), step0=0.0) == E_DIMS
    assert _call(L, ok(), up=float("nan")) == E_DIMS
    assert _call(L, ok(), down=float("inf")) == E_DIMS
    # pointers and alignment
    for missing in ("x", "params", "betas", "tail", "ws"):
        assert _call(L, ok(), **{missing: None}) == E_NULL
    assert _call(L, ok(), base=None, base_K=1) == E_NULL
    assert _call(L, ok(), base=256, base_K=0) == E_DIMS
    assert _call(L, ok(), params=260) == E_ALIGN
    assert _call(L, ok(), ws=128) == E_ALIGN
    assert _call(L, ok(), betas=258) == E_ALIGN
    # the size query refuses the same sizes, and what it admits at the gates' corners fits the LDS
    b = C.c_uint64()
    q = lambda cd, model=2, bk=0, c=16: L.lib.gmvae_ais_workspace_bytes(C.byref(cd), model, bk, c, C.byref(b))
    assert q(ok(hidden=[513])) == E_DIMS and q(ok(L=129)) == E_DIMS and q(ok(K=65)) == E_DIMS and q(ok(), c=0) == E_DIMS
    assert q(ok(sched_flags=L.OBJ_PIXEL_MASK)) == E_DIMS
    assert q(ok(D=3073, L=128, K=64, hidden=[512, 512, 512]), bk=64) == 0 and b.value > 0
    assert q(ok(hidden=[]), 0) == 0 and q(ok(L=128, hidden=[512])) == 0
    assert L.lib.gmvae_ais_workspace_bytes(C.byref(ok()), 2, 0, 16, None) == E_NULL
    n = L.ais_workspace_bytes(ok(B=8, L=64), 2, 10, 16)
    assert n == L.ais_workspace_bytes(ok(B=8, L=64, D=50000), 2, 10, 16)       # O(B C L): not a function of D ...
    assert n < 8 * 16 * 64 * 4 * 4 + 65536                                       # ... z and two gradients per chain, and change


# -------------------------------------------------------------------------------------------------------------------- flags
def test_runner_flags():
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    cfg = p.parse_args(["--mode=eval", "--ais_chains=8", "--ais_temps=100"])
    run_gmvae.check_args(p, cfg)
    assert (cfg.ais_leapfrog, cfg.ais_step_size, cfg.ais_init, cfg.ais_schedule) == (10, 0.05, "prior", "sigmoid")
    assert p.parse_args([]).ais_chains == 0
    for bad in (["--mode=eval", "--ais_chains=8"], ["--mode=eval", "--ais_temps=8"], ["--ais_chains=8", "--ais_temps=8"],
                ["--mode=eval", "--ais_chains=8", "--ais_temps=8", "--ais_leapfrog=0"],
                ["--mode=eval", "--ais_chains=8", "--ais_temps=8", "--ais_step_size=0"],
                ["--mode=eval", "--ais_chains=8", "--ais_temps=8", "--missing_rate=0.5"],
                ["--mode=eval", "--ais_chains=-1", "--ais_temps=8"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))


def test_engine_schedule():
    """Engine.ais_bound's path is the statement's; a schedule tensor is checked."""
    from gmvae_amd.engine import ais_schedule
    for kind in ("linear", "sigmoid"):
        for T in (1, 7, 1000):
            np.testing.assert_allclose(ais_schedule(kind, T).numpy(), R.schedule(kind, T), rtol=0, atol=1e-15)
    assert torch.equal(ais_schedule(torch.tensor([0.0, 0.25, 1.0]), 2), torch.tensor([0.0, 0.25, 1.0], dtype=torch.float64))
    for bad in ([0.0, 0.5, 0.5, 1.0], [0.1, 0.5, 0.7, 1.0], [0.0, 0.5, 1.0]):
        with pytest.raises(ValueError):
            ais_schedule(torch.tensor(bad), 3)
    with pytest.raises(ValueError):
        ais_schedule("cosine", 3)
