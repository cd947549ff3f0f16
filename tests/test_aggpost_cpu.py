"""CPU-side checks of gmvae_mixture_logpdf_* (include/gmvae_hip.h) and of the fp64 statement the GPU tests hold it to
(tests/aggpost_ref.py): the three names are declared, exported and bound; every failing argument returns its documented code
before any launch (fake pointers, never dereferenced); how the workspace size moves; the statement against
torch.distributions.MixtureSameFamily and against closed forms; the runner's flag checks.  No compute calls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import aggpost_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_mixture_logpdf_workspace_bytes", "gmvae_mixture_logpdf_accumulate", "gmvae_mixture_logpdf_finish"}
E_NULL, E_DIMS, E_ALIGN = -1, -2, -4
P = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def test_names_are_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\bint\s+(\w+)\s*\(", hdr))
    assert NAMES <= declared <= set(L.EXPORTS)
    raw = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and getattr(L.lib, name).argtypes is not None
    assert L.lib.gmvae_abi_version() == L.ABI_VERSION == 7


def size(L, M, Lz, per_dim):
    b = C.c_uint64()
    rc = L.lib.gmvae_mixture_logpdf_workspace_bytes(M, Lz, per_dim, C.byref(b))
    return rc, b.value


def test_workspace_size(L):
    for M in (1, 67, 1024, 10000):
        for Lz in (1, 5, 64, 128):
            rc0, b0 = size(L, M, Lz, 0)
            rc1, b1 = size(L, M, Lz, 1)
            assert rc0 == rc1 == 0 and b0 % 16 == 0 and b1 % 16 == 0
            assert b0 >= 2 * 2 * M * 16 and b1 >= 2 * (2 * M + M * Lz) * 16          # a running state and one slice, at least
            assert b1 > b0
            assert size(L, M, Lz, 0)[1] == size(L, M, 2 * Lz, 0)[1]                    # without per_dim: no state per dimension
    assert size(L, 100000, 8, 1)[1] > size(L, 10000, 8, 1)[1] > size(L, 1000, 8, 1)[1]      # grows with M
    assert size(L, 10000, 128, 1)[1] > size(L, 10000, 64, 1)[1] > size(L, 10000, 8, 1)[1]    # ... and with L under per_dim
    assert size(L, 0, 8, 1)[0] == E_DIMS and size(L, 8, 0, 1)[0] == E_DIMS and size(L, -3, 8, 0)[0] == E_DIMS
    assert size(L, (1 << 30) + 1, 8, 0)[0] == E_DIMS and size(L, 8, (1 << 16) + 1, 0)[0] == E_DIMS
    assert L.lib.gmvae_mixture_logpdf_workspace_bytes(8, 8, 1, None) == E_NULL


def accumulate(L, z=P, M=8, Lz=4, mu=P, sigma=P, logw=P, Cn=16, c_first=0, cpo=1, owner=None, per_dim=1, ws=P):
    ptr = lambda a: None if a is None else C.c_void_p(a)
    return L.lib.gmvae_mixture_logpdf_accumulate(ptr(z), M, Lz, ptr(mu), ptr(sigma), ptr(logw), Cn, c_first, cpo, ptr(owner),
                                                 per_dim, ptr(ws), None)


def finish(L, M=8, Lz=4, per_dim=1, joint=P, dim=P, own=P, ws=P):
    ptr = lambda a: None if a is None else C.c_void_p(a)
    return L.lib.gmvae_mixture_logpdf_finish(M, Lz, per_dim, 0.0, ptr(joint), ptr(dim), ptr(own), ptr(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for per_dim in (0, 1):
        a = lambda **kw: accumulate(L, per_dim=per_dim, **kw)
        for name in ("z", "mu", "sigma", "logw", "ws"):
            assert a(**{name: None}) == E_NULL, name
        assert a(M=0) == E_DIMS and a(Lz=0) == E_DIMS and a(Cn=0) == E_DIMS and a(M=-1) == E_DIMS and a(Cn=-5) == E_DIMS
        assert a(M=(1 << 30) + 1) == E_DIMS and a(Cn=(1 << 30) + 1) == E_DIMS and a(Lz=(1 << 16) + 1) == E_DIMS
        assert a(c_first=-1) == E_DIMS
        assert a(owner=P, cpo=0) == E_DIMS and a(owner=P, cpo=-2) == E_DIMS
        assert a(z=None, M=0) == E_DIMS                                   # the sizes come first,
        assert a(ws=None, z=P + 2) == E_NULL                              # then NULL, then the alignment
        for name in ("z", "mu", "sigma", "logw"):
            assert a(**{name: P + 2}) == E_ALIGN, name
        assert a(owner=P + 4) == E_ALIGN and a(ws=P + 8) == E_ALIGN
        f = lambda **kw: finish(L, per_dim=per_dim, **kw)
        assert f(ws=None) == E_NULL and f(M=0) == E_DIMS and f(Lz=0) == E_DIMS and f(M=0, ws=None) == E_DIMS
        for name in ("joint", "dim", "own"):
            assert f(**{name: P + 2}) == E_ALIGN, name
        assert f(ws=P + 8) == E_ALIGN


def _case(seed, M, Cn, Lz):
    rng = np.random.default_rng(seed)
    mu, sigma = rng.normal(0, 1, (Cn, Lz)), rng.uniform(0.3, 1.5, (Cn, Lz))
    logw = np.log(rng.dirichlet(np.ones(Cn)))
    return rng.normal(0, 1.5, (M, Lz)), mu, sigma, logw


def test_the_statement_is_mixture_same_family():
    import torch
    from torch import distributions as D
    for seed, (M, Cn, Lz) in enumerate([(1, 1, 1), (3, 5, 2), (17, 30, 5), (9, 40, 64)]):
        z, mu, sigma, logw = _case(seed, M, Cn, Lz)
        ref = R.mixture_logpdf(z, mu, sigma, logw)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        cat = D.Categorical(logits=t(logw))
        joint = D.MixtureSameFamily(cat, D.Independent(D.Normal(t(mu), t(sigma)), 1)).log_prob(t(z))
        np.testing.assert_allclose(ref["log_joint"], joint.numpy(), rtol=1e-12, atol=1e-12)
        for d in range(Lz):
            dim = D.MixtureSameFamily(cat, D.Normal(t(mu[:, d]), t(sigma[:, d]))).log_prob(t(z[:, d]))
            np.testing.assert_allclose(ref["log_dim"][:, d], dim.numpy(), rtol=1e-12, atol=1e-12)
        # own: the same mixture cut down to the owner's components, weights not renormalised
        cpo = 2 if Cn > 1 else 1
        owner = np.random.default_rng(seed).integers(0, (Cn + cpo - 1) // cpo, M)
        own = R.mixture_logpdf(z, mu, sigma, logw, 0.7, cpo, owner)
        np.testing.assert_allclose(own["log_joint"], ref["log_joint"] - 0.7, rtol=1e-12, atol=1e-12)
        for m in range(M):
            sl = slice(owner[m] * cpo, min(Cn, (owner[m] + 1) * cpo))
            one = R.mixture_logpdf(z[m:m + 1], mu[sl], sigma[sl], logw[sl])["log_joint"][0]
            assert own["log_own"][m] == pytest.approx(one, rel=1e-12, abs=1e-12)


def test_closed_forms_and_the_empty_cases():
    rng = np.random.default_rng(3)
    for Lz in (1, 5, 64):
        z = rng.normal(0, 2, (7, Lz))
        one = R.mixture_logpdf(z, np.zeros((1, Lz)), np.ones((1, Lz)), np.zeros(1))
        np.testing.assert_allclose(one["log_joint"], -0.5 * (z * z).sum(1) - 0.5 * Lz * math.log(2 * math.pi), rtol=1e-13)
        np.testing.assert_allclose(one["log_dim"], -0.5 * z * z - 0.5 * math.log(2 * math.pi), rtol=1e-13)
    # a -inf component contributes nothing and yields no NaN; all of them -inf give -inf
    z, mu, sigma, logw = _case(5, 4, 6, 3)
    cut = logw.copy()
    cut[[1, 4]] = -np.inf
    keep = [0, 2, 3, 5]
    a, b = R.mixture_logpdf(z, mu, sigma, cut), R.mixture_logpdf(z, mu[keep], sigma[keep], logw[keep])
    np.testing.assert_allclose(a["log_joint"], b["log_joint"], rtol=1e-13)
    np.testing.assert_allclose(a["log_dim"], b["log_dim"], rtol=1e-13)
    none = R.mixture_logpdf(z, mu, sigma, np.full(6, -np.inf), 0.0, 2, np.zeros(4, np.int64))
    assert np.all(none["log_joint"] == -np.inf) and np.all(none["log_dim"] == -np.inf) and np.all(none["log_own"] == -np.inf)
    # far queries stay finite
    far = R.mixture_logpdf(z + 50.0, mu, np.full_like(sigma, 0.01), logw)
    assert np.all(np.isfinite(far["log_joint"])) and far["log_joint"].max() < -1e7


def test_mutual_information_closed_forms():
    rng = np.random.default_rng(8)
    N, Lz = 12, 4
    # N identical examples: q(z) = q(z | x), mi = 0 at every sample
    mu, sigma = np.tile(rng.normal(0, 1, (1, 1, Lz)), (N, 1, 1)), np.tile(rng.uniform(0.5, 1.0, (1, 1, Lz)), (N, 1, 1))
    z = mu[:, 0] + sigma[:, 0] * rng.normal(0, 1, (N, Lz))
    same = R.decomposition(np.zeros((N, 1)), mu, sigma, z, np.arange(N), None)
    assert abs(same["mi"]) < 1e-12 and np.abs(same["log_q_zx"] - same["log_q_z"]).max() < 1e-12
    assert same["kl_avg"] == pytest.approx(same["mi"] + same["kl_marginal"], abs=1e-12) and same["active_units"] == 0
    # N well separated sharp examples: q(z) = q(z | x) / N at every sample, mi -> ln N
    mu = (10.0 * np.arange(N))[:, None, None] * np.ones((1, 1, Lz))
    sigma = np.full((N, 1, Lz), 0.05)
    z = mu[:, 0] + sigma[:, 0] * rng.normal(0, 1, (N, Lz))
    apart = R.decomposition(np.zeros((N, 1)), mu, sigma, z, np.arange(N), None)
    assert apart["mi"] == pytest.approx(math.log(N), abs=1e-12) and apart["active_units"] == Lz
    assert np.all(apart["log_q_zx"] - apart["log_q_z"] <= math.log(N) + 1e-12)
    assert apart["kl_avg"] == pytest.approx(apart["mi"] + apart["kl_marginal"], rel=1e-12)
    # K components per example, a mixture prior: the identity holds, the y terms are those of the weights
    K = 3
    logpi = np.log(rng.dirichlet(np.ones(K), N))
    mu, sigma = rng.normal(0, 1, (N, K, Lz)), rng.uniform(0.3, 1.0, (N, K, Lz))
    qidx = np.array([0, 5, 5, 11, 2])
    z = mu[qidx, 1] + sigma[qidx, 1] * rng.normal(0, 1, (5, Lz))
    pr = (np.log(np.full(K, 1.0 / K)), rng.normal(0, 1, (K, Lz)), rng.uniform(0.5, 1.5, (K, Lz)))
    g = R.decomposition(logpi, mu, sigma, z, qidx, pr)
    assert g["kl_avg"] == pytest.approx(g["mi"] + g["kl_marginal"], rel=1e-12)
    assert np.all(g["log_q_zx"] - g["log_q_z"] <= math.log(N) + 1e-12)
    pi = np.exp(logpi)
    assert g["mi_xy"] == pytest.approx((pi * (logpi - np.log(pi.mean(0)))).sum(1).mean(), rel=1e-12)      # E_x KL(pi_x || q_y)
    assert 0 <= g["mi_xy"] <= g["q_y_entropy"] <= math.log(K) + 1e-12


def test_runner_flag_checks(L):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--latent_diagnostics=64"]))
    assert ok.latent_diagnostics == 64
    assert run_gmvae.check_args(p, p.parse_args(["--mode=train"])).latent_diagnostics == 0
    for bad in (["--mode=train", "--latent_diagnostics=64"], ["--latent_diagnostics=64"],
                ["--mode=eval", "--latent_diagnostics=64", "--missing_rate=0.2"], ["--mode=eval", "--latent_diagnostics=-1"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
