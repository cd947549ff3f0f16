"""CPU-side checks of gmvae_mixfit_full_* (include/gmvae_hip.h) and of the fp64 statement the GPU tests hold it to
(tests/mixfit_full_ref.py): the three names are declared, exported and bound; the workspace's size is the header's formula; every
failing argument returns its documented code before any launch (fake pointers, never dereferenced), in the documented order; the
runner's flag checks; the statement against scikit-learn's 'full' functions and against the diagonal statement; the info rule; the
striped case on which the diagonal fit fails and the full one does not.  No compute calls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mixfit_full_ref as F
import mixfit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_mixfit_full_workspace_bytes", "gmvae_mixfit_full_assign", "gmvae_mixfit_full_run"}
E_NULL, E_DIMS, E_ALIGN = -1, -2, -4
P = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch
SHAPES = [(1, 1, 1), (67, 5, 3), (403, 16, 4), (1031, 64, 10), (259, 67, 3), (130, 128, 8), (2050, 2, 256), (300, 64, 256),
          (16453, 19, 2)]      # tests/test_mixfit_full.py's


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


def size(L, N, Lz, K):
    b = C.c_uint64()
    return L.lib.gmvae_mixfit_full_workspace_bytes(N, Lz, K, C.byref(b)), b.value


def header_formula(N, Lz, K):
    """include/gmvae_hip.h: (bytes, row slices G, rows per tile T)."""
    Pk = Lz * (Lz + 1) // 2
    stride = K * (Pk + Lz + 1) + 1
    T = min(64, (163840 - 8 * (Pk + Lz)) // (8 * ((Lz | 1) + (K | 1) + 3) + 4 * (Lz | 1))) // 4 * 4
    tiles = -(-N // T)
    g = min(tiles, 256, (1 << 23) // stride)
    per = -(-tiles // g) * T
    G = -(-N // per)
    return -(-8 * (K * Pk + K + G * stride) // 16) * 16, G, T


BAD_SIZES = [(0, 4, 3), (-5, 4, 3), ((1 << 24) + 1, 4, 3), (64, 0, 3), (64, 129, 1), (64, 4, 0), (64, 4, 257), (64, 64, 257),
             (64, 128, 65), (64, 65, 256), (64, 4096, 1)]


def test_workspace_size_is_the_header_s_formula(L):
    for shape in SHAPES + [(60000, 64, 10), (10000, 64, 10), (1 << 24, 128, 64), (1 << 24, 1, 1), (1 << 24, 64, 256), (5, 128, 64)]:
        rc, b = size(L, *shape)
        want, G, T = header_formula(*shape)
        assert rc == 0 and b == want and b % 16 == 0, (shape, b, want)
        assert 1 <= G <= 256 and T >= 4 and T % 4 == 0
        N, Lz, K = shape
        assert G * (K * (Lz * (Lz + 1) // 2 + Lz + 1) + 1) <= 1 << 23                       # 64 MiB of partial sums at most
    assert size(L, 1 << 24, 64, 10)[1] == size(L, 1 << 23, 64, 10)[1]                      # nothing per row
    assert size(L, 64, 128, 64)[0] == 0 and size(L, 64, 64, 256)[0] == 0                   # K L^2 = 2^20 is inside the gate
    for bad in BAD_SIZES:
        assert size(L, *bad)[0] == E_DIMS, bad
    assert L.lib.gmvae_mixfit_full_workspace_bytes(8, 8, 2, None) == E_NULL
    assert L.lib.gmvae_mixfit_full_workspace_bytes(0, 8, 2, None) == E_DIMS                # the sizes come first
    from gmvae_amd import mixfit
    assert mixfit.full_workspace_bytes(1031, 64, 10) == header_formula(1031, 64, 10)[0]


def _p(a):
    return None if a is None else C.c_void_p(a)


def assign(L, codes=P, N=64, Lz=4, K=3, logw=P, mu=P, cov=P, log_resp=P, lse=P, info=P, ws=P):
    return L.lib.gmvae_mixfit_full_assign(_p(codes), N, Lz, K, _p(logw), _p(mu), _p(cov), _p(log_resp), _p(lse), _p(info), _p(ws), None)


def run(L, codes=P, N=64, Lz=4, K=3, logw=P, mu=P, cov=P, reg=1e-6, n_iter=3, hist=P, counts=P, info=P, ws=P):
    return L.lib.gmvae_mixfit_full_run(_p(codes), N, Lz, K, _p(logw), _p(mu), _p(cov), reg, n_iter, _p(hist), _p(counts), _p(info),
                                       _p(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for fn, ptrs, optional in ((assign, ("codes", "logw", "mu", "cov", "ws"), ("log_resp", "lse", "info")),
                               (run, ("codes", "logw", "mu", "cov", "ws"), ("hist", "counts", "info"))):
        f = lambda **kw: fn(L, **kw)
        for N, Lz, K in BAD_SIZES:
            assert f(N=N, Lz=Lz, K=K) == E_DIMS, (fn.__name__, N, Lz, K)
        for name in ptrs:
            assert f(**{name: None}) == E_NULL, (fn.__name__, name)
            assert f(**{name: None}, N=0) == E_DIMS, (fn.__name__, name)                       # the sizes come first,
            other = ptrs[0] if name != ptrs[0] else ptrs[1]
            assert f(**{name: None, other: P + 2}) == E_NULL, (fn.__name__, name)              # then NULL, then the alignment
            assert f(**{name: P + (8 if name == "ws" else 2)}) == E_ALIGN, (fn.__name__, name)
        for name in optional:
            assert f(**{name: P + 2}) == E_ALIGN, (fn.__name__, name)
            assert f(**{name: None, "codes": None}) == E_NULL, (fn.__name__, name)             # (NULL there is no error of its own)
    for reg in (0.0, -1e-6, float("nan"), float("inf")):
        assert run(L, reg=reg) == E_DIMS and run(L, reg=reg, codes=None) == E_DIMS, reg
    assert run(L, n_iter=-1) == E_DIMS and run(L, n_iter=-1, codes=None) == E_DIMS
    # the gates on the compute entry points: K L^2 = 2^20 passes the size check (and fails the next one), one more component does not
    assert assign(L, Lz=128, K=64, codes=None) == E_NULL and assign(L, Lz=128, K=65, codes=None) == E_DIMS
    assert run(L, Lz=64, K=256, codes=None) == E_NULL and run(L, Lz=129, K=1, codes=None) == E_DIMS
    # n_iter = 0 with every argument in order is a valid call that launches nothing
    assert run(L, n_iter=0, hist=None, counts=None, info=None) == 0


def test_runner_flag_checks(L, monkeypatch):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64", "--mixture_covariance=full", "--mixture_bic",
                                               "--latent_size=128"]))
    assert (ok.fit_latent_mixture, ok.mixture_covariance, ok.mixture_bic) == (64, "full", True)
    plain = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64"]))
    assert (plain.mixture_covariance, plain.mixture_bic) == ("diag", False)
    run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64", "--mixture_bic"]))      # either covariance
    run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64", "--latent_size=129"]))  # the diagonal fit's gate
    for bad in (["--mode=eval", "--mixture_covariance=full"],
                ["--mode=eval", "--fit_latent_mixture=64", "--mixture_covariance=full", "--latent_size=129"],
                ["--mode=eval", "--mixture_bic"],
                ["--mode=eval", "--fit_latent_mixture=64", "--mixture_covariance=tied"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))


# ------------------------------------------------------------------------------------------------------------ the statement
def spd(rng, K, Lz, lo=0.05, hi=3.0):
    """cov_k = Q diag(s^2) Q^T, s uniform in [lo, hi], as fp32 values."""
    out = np.zeros((K, Lz, Lz), np.float32)
    for k in range(K):
        q, _ = np.linalg.qr(rng.normal(0, 1, (Lz, Lz)))
        out[k] = ((q * rng.uniform(lo, hi, Lz) ** 2) @ q.T).astype(np.float32)
    return out


def test_statement_agrees_with_scikit_learn():
    """mixfit_full_ref (without the fp32 rounding of the parameters, which is the ABI's and not scikit-learn's) against
    sklearn.mixture._gaussian_mixture with 'full' at N = 203, L = 5, K = 3 over 5 iterations: l within 1e-7, mu', cov' and logw'
    within 1e-10 in every iteration."""
    pytest.importorskip("sklearn")
    from sklearn.mixture import _gaussian_mixture as G
    z, lab = R.blobs(203, 5, 3, 0, sep=2.0)
    z = z.astype(np.float64)
    logw, mu, cov = F.start(z, R.first_of_each(lab, 3))
    worst = dict(l=0.0, mu=0.0, cov=0.0, logw=0.0)
    for _ in range(5):
        l, lse, lr, info = F.estep(z, logw, mu, cov)
        assert not info.any()
        l_sk = G._estimate_log_gaussian_prob(z, mu, G._compute_precision_cholesky(cov, "full"), "full") + logw
        nk, means, covs = G._estimate_gaussian_parameters(z, np.exp(lr), 1e-6, "full")
        logw2, mu2, cov2, counts = F.mstep(z, lr, mu, 1e-6)
        assert counts.min() > 1.0
        for k, v in (("l", np.abs(l - l_sk).max()), ("mu", np.abs(mu2 - means).max()), ("cov", np.abs(cov2 - covs).max()),
                     ("logw", np.abs(logw2 - np.log(nk / nk.sum())).max())):
            worst[k] = max(worst[k], float(v))
        logw, mu, cov = logw2, mu2, cov2
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["l"] <= 1e-7 and max(worst["mu"], worst["cov"], worst["logw"]) <= 1e-10
    for K, Lz in ((3, 5), (10, 64), (1, 1), (256, 2)):
        for ct in ("full", "diag"):
            gm = G.GaussianMixture(n_components=K, covariance_type=ct)
            gm.means_ = np.zeros((K, Lz))
            assert F.n_parameters(K, Lz, ct) == gm._n_parameters()


def test_n_parameters_and_information_criteria(L):
    from gmvae_amd import mixfit
    import torch
    for K, Lz in ((3, 5), (10, 64), (1, 1), (256, 2)):
        assert mixfit.n_parameters(K, Lz, "diag") == K - 1 + 2 * K * Lz == F.n_parameters(K, Lz, "diag")
        assert mixfit.n_parameters(K, Lz, "full") == K - 1 + K * Lz + K * Lz * (Lz + 1) // 2 == F.n_parameters(K, Lz, "full")
    with pytest.raises(ValueError):
        mixfit.n_parameters(3, 5, "tied")
    ll = torch.tensor(-10.125, dtype=torch.float64)
    full = {"loglik": ll, "mu": torch.zeros(3, 5), "cov": torch.zeros(3, 5, 5)}
    diag = {"loglik": ll, "mu": torch.zeros(3, 5), "sigma": torch.zeros(3, 5)}
    assert mixfit.bic(full, 402).item() == pytest.approx(2 * 402 * 10.125 + 62 * math.log(402), rel=1e-14)
    assert mixfit.bic(diag, 402).item() == pytest.approx(2 * 402 * 10.125 + 32 * math.log(402), rel=1e-14)
    assert mixfit.aic(full, 402).item() == pytest.approx(2 * 402 * 10.125 + 2 * 62, rel=1e-14)
    assert mixfit.aic(diag, 402).item() == pytest.approx(2 * 402 * 10.125 + 2 * 32, rel=1e-14)


def test_with_diagonal_covariances_the_e_step_is_the_diagonal_statement_s():
    rng = np.random.default_rng(3)
    for N, Lz, K in ((67, 5, 3), (130, 64, 10)):
        z = rng.normal(0, 1, (N, Lz)).astype(np.float32)
        mu = z[rng.integers(0, N, K)].copy()
        sigma = rng.uniform(0.05, 3.0, (K, Lz))
        logw = rng.normal(0, 1, K)
        logw[1] = -np.inf
        cov = np.stack([np.diag(s * s) for s in sigma])
        l, lse, lr, info = F.estep(z, logw, mu, cov)
        l0, lse0, lr0 = R.estep(z, logw, mu, sigma)
        fin = np.isfinite(l0)
        err = max(float((np.abs(l[fin] - l0[fin]) / np.maximum(1.0, np.abs(l0[fin]))).max()), float(np.abs(lse - lse0).max() / max(1.0, np.abs(lse0).max())),
                  float(np.abs(lr[fin] - lr0[fin]).max()))
        print((N, Lz, K), f"{err:.2e}")
        assert err <= 1e-12 and not info.any() and np.array_equal(np.isneginf(lr), np.isneginf(lr0)) and not np.isnan(lr).any()


def test_the_info_rule():
    rng = np.random.default_rng(4)
    z = rng.normal(0, 1, (31, 3)).astype(np.float32)
    mu = z[:2].copy()
    logw = np.log(np.array([0.5, 0.5]))
    good = spd(rng, 1, 3)[0].astype(np.float64)
    # diag(1, 0.5, -1): the third pivot is negative
    cov = np.stack([np.diag([1.0, 0.5, -1.0]), good])
    # an exact 0 pivot at j = 1: a_11 - C_10^2 = 4 - 2^2
    zero = np.array([[1.0, 0, 0], [2.0, 4.0, 0], [0.5, 0.25, 9.0]])
    # a NaN pivot at j = 0
    nan = np.diag([np.nan, 1.0, 1.0])
    for bad, want in ((np.diag([1.0, 0.5, -1.0]), 3), (zero, 2), (nan, 1), (np.diag([0.0, 1.0, 1.0]), 1)):
        for dtype in (np.float64, np.float32):
            cov = np.stack([bad, good])
            C_, info = F.factor(cov, dtype)
            assert info.tolist() == [want, 0], (want, info)
            l, lse, lr, info = F.estep(z, logw, mu, cov, dtype)
            assert info.tolist() == [want, 0]
            assert np.isneginf(l[:, 0]).all() and np.isneginf(lr[:, 0]).all() and np.isfinite(lse).all()
            assert not np.isnan(l).any() and not np.isnan(lr).any() and np.allclose(lr[:, 1], 0.0, atol=1e-6)
            logw2, mu2, cov2, counts = F.mstep(z, lr, mu, 1e-6, dtype)
            assert counts[0] == 0 and np.array_equal(mu2[0], mu[0].astype(dtype)) and np.allclose(cov2[0], 1e-6 * np.eye(3), rtol=1e-6, atol=0)
            assert all(np.isfinite(a).all() for a in (logw2, mu2, cov2))
    # only the lower triangle is read
    upper = good.copy()
    upper[np.triu_indices(3, 1)] = np.nan
    assert np.array_equal(F.factor(upper[None])[0], F.factor(good[None])[0])
    assert np.allclose(F.factor(good[None])[0][0], np.linalg.cholesky(good), rtol=1e-12)


def test_every_component_absent_gives_minus_infinity_and_no_nan():
    z = np.zeros((5, 2), np.float32)
    l, lse, lr, info = F.estep(z, np.zeros(1), np.zeros((1, 2)), -np.eye(2)[None])
    assert info.tolist() == [1] and np.isneginf(lse).all() and np.isneginf(lr).all()
    o = F.fit(z + np.arange(5, dtype=np.float32)[:, None], np.zeros(1), np.zeros((1, 2)), -np.eye(2)[None], 2)
    assert o["info"].tolist() == [1] and all(np.isfinite(o[k]).all() for k in ("logw", "mu", "cov"))      # positive definite again


STRIPES = dict(N=402, L=5, K=3, seed=7, gap=8, length=8)


def test_the_striped_case_needs_full_covariances():
    """Three parallel elongated clusters: from the same start, 60 iterations of the full statement recover every label and the
    diagonal statement does not (measured: accuracy 1.0 against 0.43, log-likelihood -10.133 against -10.948)."""
    z, lab = F.stripes(**STRIPES)
    idx = R.first_of_each(lab, 3)
    full = F.fit(z, *F.start(z, idx), 60)
    diag = R.fit(z, *R.start(z, idx), 60)
    acc_f, acc_d = R.cluster_acc(full["log_resp"], lab), R.cluster_acc(diag["log_resp"], lab)
    print(f"full: accuracy {acc_f}, loglik {full['loglik']:.4f}; diag: accuracy {acc_d:.3f}, loglik {diag['loglik']:.4f}")
    assert acc_f == 1.0 and acc_d <= 0.6 and full["loglik"] - diag["loglik"] >= 0.5 and not full["info"].any()
    h = np.append(full["loglik_history"], full["loglik"])
    assert np.all(np.diff(h) >= -1e-6)                                                     # (the parameters are rounded to fp32)
    # the first E-step is the diagonal fit's
    assert abs(full["loglik_history"][0] - diag["loglik_history"][0]) <= 1e-6
    # the fp32 rounding of the parameters moves the result by about 1e-6, no more
    f32 = F.fit(z, *F.start(z, idx), 60, dtype=np.float32)
    dev = max(float((np.abs(f32[k] - full[k]) / np.maximum(1.0, np.abs(full[k]))).max()) for k in ("logw", "mu", "cov"))
    print(f"the fp32 statement's deviation after 60 iterations: {dev:.2e}")
    assert dev <= 1e-3
