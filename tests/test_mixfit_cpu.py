"""CPU-side checks of gmvae_mixfit_* (include/gmvae_hip.h) and of the fp64 statement the GPU tests hold it to
(tests/mixfit_ref.py): the three names are declared, exported and bound; every failing argument returns its documented code before
any launch (fake pointers, never dereferenced), in the documented order; the workspace's size; the runner's flag checks; the
statement against scikit-learn's _estimate_log_gaussian_prob / _estimate_gaussian_parameters; the statement's own properties.
No compute calls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mixfit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_mixfit_workspace_bytes", "gmvae_mixfit_assign", "gmvae_mixfit_run"}
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


def size(L, N, Lz, K):
    b = C.c_uint64()
    return L.lib.gmvae_mixfit_workspace_bytes(N, Lz, K, C.byref(b)), b.value


BAD_SIZES = [(0, 4, 3), (-5, 4, 3), ((1 << 24) + 1, 4, 3), (64, 0, 3), (64, 4097, 1), (64, 4, 0), (64, 4, 257), (64, 129, 128),
             (64, 128, 129), (64, 4096, 5)]


def test_workspace_size(L):
    for N in (1, 67, 1024, 60000, 1 << 24):
        for Lz, K in ((1, 1), (5, 3), (64, 10), (67, 65), (128, 128), (2, 256), (4096, 4)):
            rc, b = size(L, N, Lz, K)
            assert rc == 0 and b % 16 == 0 and b >= 16, (N, Lz, K)
            # at most 256 workgroups' K (2 L + 1) + 1 fp64 values; nothing per row, so nothing grows with N beyond that
            assert b <= 256 * (K * (2 * Lz + 1) + 1) * 8 + 16 + 8 * N, (N, Lz, K, b)
            assert b >= (K * (2 * Lz + 1) + 1) * 8
    assert size(L, 1 << 24, 64, 10)[1] == size(L, 1 << 23, 64, 10)[1]
    assert size(L, 64, 128, 128)[0] == 0 and size(L, 64, 4096, 4)[0] == 0            # K L = 16,384 is inside the gate
    for bad in BAD_SIZES:
        assert size(L, *bad)[0] == E_DIMS, bad
    assert L.lib.gmvae_mixfit_workspace_bytes(8, 8, 2, None) == E_NULL
    assert L.lib.gmvae_mixfit_workspace_bytes(0, 8, 2, None) == E_DIMS               # the sizes come first


def _p(a):
    return None if a is None else C.c_void_p(a)


def assign(L, codes=P, N=64, Lz=4, K=3, logw=P, mu=P, sigma=P, log_resp=P, lse=P, ws=P):
    return L.lib.gmvae_mixfit_assign(_p(codes), N, Lz, K, _p(logw), _p(mu), _p(sigma), _p(log_resp), _p(lse), _p(ws), None)


def run(L, codes=P, N=64, Lz=4, K=3, logw=P, mu=P, sigma=P, reg=1e-6, n_iter=3, hist=P, counts=P, ws=P):
    return L.lib.gmvae_mixfit_run(_p(codes), N, Lz, K, _p(logw), _p(mu), _p(sigma), reg, n_iter, _p(hist), _p(counts), _p(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for fn, ptrs, optional in ((assign, ("codes", "logw", "mu", "sigma", "ws"), ("log_resp", "lse")),
                               (run, ("codes", "logw", "mu", "sigma", "ws"), ("hist", "counts"))):
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
    for reg in (0.0, -1e-6, float("nan"), float("inf")):
        assert run(L, reg=reg) == E_DIMS and run(L, reg=reg, codes=None) == E_DIMS, reg
    assert run(L, n_iter=-1) == E_DIMS and run(L, n_iter=-1, codes=None) == E_DIMS
    # the K L gate on the compute entry points: 16,384 passes the size check (and fails the next one), 129 x 128 does not
    assert assign(L, Lz=128, K=128, codes=None) == E_NULL and assign(L, Lz=128, K=129, codes=None) == E_DIMS
    assert run(L, Lz=128, K=128, codes=None) == E_NULL and run(L, Lz=129, K=128, codes=None) == E_DIMS
    # n_iter = 0 with every argument in order is a valid call that launches nothing
    assert run(L, n_iter=0, hist=None, counts=None) == 0


def test_runner_flag_checks(L, monkeypatch):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64", "--mixture_fit_iters=20",
                                               "--mixture_fit_inits=3"]))
    assert (ok.fit_latent_mixture, ok.mixture_fit_iters, ok.mixture_fit_inits) == (64, 20, 3)
    plain = run_gmvae.check_args(p, p.parse_args(["--mode=eval"]))
    assert (plain.fit_latent_mixture, plain.mixture_fit_iters, plain.mixture_fit_inits) == (0, 100, 1)
    run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--model=vae", "--fit_latent_mixture=10"]))      # N = K is enough
    run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64", "--mixture_fit_iters=0"]))
    for bad in (["--mode=train", "--fit_latent_mixture=64"], ["--fit_latent_mixture=64"], ["--mode=eval", "--fit_latent_mixture=-1"],
                ["--mode=eval", "--fit_latent_mixture=9"],                           # fewer codes than the 10 default components
                ["--mode=eval", "--fit_latent_mixture=64", "--mixture_components=65"],
                ["--mode=eval", "--fit_latent_mixture=64", "--mixture_fit_iters=-1"],
                ["--mode=eval", "--fit_latent_mixture=64", "--mixture_fit_inits=0"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--fit_latent_mixture=64"]))
    run_gmvae.check_args(p, p.parse_args(["--mode=eval"]))                  # without the flag, several ranks are fine


blobs, first_of_each = R.blobs, R.first_of_each


def test_statement_agrees_with_scikit_learn():
    """mixfit_ref against sklearn.mixture._gaussian_mixture at N = 203, L = 5, K = 3 after 5 iterations, no component empty: l_nk
    within 1e-13 max(1, |ref|), the M-step's means and sigma within 1e-12, logw equal to 1e-14."""
    pytest.importorskip("sklearn")
    from sklearn.mixture import _gaussian_mixture as G
    z, lab = blobs(203, 5, 3, 0, sep=2.0)
    z = z.astype(np.float64)
    logw, mu, sigma = R.start(z, first_of_each(lab, 3))
    for _ in range(5):
        _, _, lr = R.estep(z, logw, mu, sigma)
        logw, mu, sigma, counts = R.mstep(z, lr, mu, 1e-6)
    assert counts.min() > 1.0                                                    # (the centred mean differs from scikit-learn's
    l, lse, lr = R.estep(z, logw, mu, sigma)                                     # only at an empty component)
    l_sk = G._estimate_log_gaussian_prob(z, mu, 1.0 / sigma, "diag") + logw
    nk, means, var = G._estimate_gaussian_parameters(z, np.exp(lr), 1e-6, "diag")
    logw2, mu2, sigma2, R2 = R.mstep(z, lr, mu, 1e-6)
    errs = {"l": np.abs(l - l_sk).max() / max(1.0, np.abs(l_sk).max()), "mu": np.abs(mu2 - means).max(),
            "sigma": np.abs(sigma2 - np.sqrt(var)).max(), "logw": np.abs(logw2 - np.log(nk / nk.sum())).max(),
            "counts": np.abs(R2 + R.EPS0 - nk).max()}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["l"] <= 1e-13 and errs["mu"] <= 1e-12 and errs["sigma"] <= 1e-12 and errs["logw"] <= 1e-14 and errs["counts"] <= 1e-12
    assert np.abs(np.exp(lr).sum(axis=1) - 1).max() < 1e-14 and np.abs(lse - np.log(np.exp(l_sk).sum(axis=1))).max() < 1e-12


def test_history_is_non_decreasing_and_the_labels_are_recovered():
    for seed, (N, Lz, K) in enumerate(((203, 5, 3), (400, 16, 4), (150, 2, 6))):
        z, lab = blobs(N, Lz, K, seed)
        o = R.fit(z, *R.start(z, first_of_each(lab, K)), 30)
        h = np.append(o["loglik_history"], o["loglik"])
        print((N, Lz, K), f"loglik {h[0]:.4f} -> {h[-1]:.4f}, smallest step {np.diff(h).min():.2e}")
        assert np.all(np.diff(h) >= -1e-12 * np.abs(h[:-1]))
        assert abs(np.exp(o["logw"]).sum() - 1) < 1e-12 and np.isfinite(o["sigma"]).all() and (o["sigma"] >= 1e-3).all()
    z, lab = blobs(400, 16, 4, 400, sep=0.0, offset=50.0)
    logw, mu, sigma = R.start(z, first_of_each(lab, 4))                       # one code per cluster, unit scales: the GPU trajectory's init
    o = R.fit(z, logw, mu, np.ones_like(sigma), 30)
    h = np.append(o["loglik_history"], o["loglik"])
    assert R.cluster_acc(o["log_resp"], lab) == 1.0 and np.all(np.diff(h) >= -1e-12 * np.abs(h[:-1]))


def test_an_empty_component_keeps_its_mean_and_yields_no_nan():
    z, lab = blobs(67, 5, 3, 5)
    logw, mu, sigma = R.start(z, first_of_each(lab, 3))
    logw = np.array([math.log(0.5), -math.inf, math.log(0.5)])
    l, lse, lr = R.estep(z, logw, mu, sigma)
    assert np.isfinite(lse).all() and (lr[:, 1] == -math.inf).all() and not np.isnan(lr).any()
    logw2, mu2, sigma2, counts = R.mstep(z, lr, mu, 1e-6)
    assert counts[1] == 0 and np.array_equal(mu2[1], mu[1].astype(np.float64)) and np.allclose(sigma2[1], 1e-3, rtol=1e-12)
    assert abs(math.exp(logw2[1]) - R.EPS0 / 67) < 1e-3 * R.EPS0 / 67 and np.isfinite(logw2).all()
    # ... in fp32 too
    _, lse32, lr32 = R.estep(z, logw, mu, sigma, np.float32)
    assert np.isfinite(lse32).all() and not np.isnan(lr32).any()


def test_centred_m_step_survives_an_offset_that_the_uncentred_one_does_not():
    """Clusters 1000 apart in one dimension: the centred M-step's sigma is the two-pass value to 1e-10 -- in fp64 by a wide margin,
    and its fp32 evaluation stays within 1e-4 of it; sum r z^2 / R - mean^2 in fp32 does not, which is why the kernel may not use it."""
    z, lab = blobs(400, 16, 4, 7, sep=0.0, offset=1000.0)
    logw, mu, sigma = R.start(z, first_of_each(lab, 4))
    sigma = np.ones_like(sigma)
    _, _, lr = R.estep(z, logw, mu, sigma)
    assert R.cluster_acc(lr, lab) == 1.0
    r = np.exp(lr)
    z64 = z.astype(np.float64)
    mean = (r[:, :, None] * z64[:, None, :]).sum(0) / (r.sum(0) + R.EPS0)[:, None]
    two_pass = np.sqrt((r[:, :, None] * (z64[:, None, :] - mean[None]) ** 2).sum(0) / (r.sum(0) + R.EPS0)[:, None] + 1e-6)
    centred = R.mstep(z, lr, mu, 1e-6)[2]
    centred32 = R.mstep(z, lr, mu, 1e-6, np.float32)[2]
    naive32 = R.mstep_uncentred(z, lr, 1e-6, np.float32)[2]
    e64, e32, en = (float(np.abs(s - two_pass).max()) for s in (centred, centred32, naive32))
    print(f"centred fp64 {e64:.2e}, centred fp32 {e32:.2e}, uncentred fp32 {en:.2e} (sigma about {two_pass.mean():.2f})")
    assert e64 <= 1e-10 and e32 <= 1e-4 and en > 1e-2


def test_seeding_statement():
    z, _ = blobs(403, 16, 4, 11)
    u = np.array([0.5, 0.25, 0.999999, 0.0], np.float32)
    idx, margin = R.kmeanspp(z, 4, u)
    assert idx[0] == 201 and len(set(idx.tolist())) == 4 and 0 < margin < 1
    same = np.repeat(z[:1], 9, axis=0)                       # every distance 0: the fallback index
    idx, margin = R.kmeanspp(same, 3, np.array([0.0, 0.5, 0.99], np.float32))
    assert idx.tolist() == [0, 4, 8] and margin == math.inf
    logw, mu, sigma = R.start(z, [3, 2, 1, 0])
    assert np.allclose(logw, -math.log(4)) and np.array_equal(mu[0], z[3].astype(np.float64)) and np.allclose(sigma[2], z.astype(np.float64).std(0))
