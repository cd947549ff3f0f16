"""gmvae_mixfit_full_* (include/gmvae_hip.h; csrc/mixfit_full.hpp) and gmvae_amd.mixfit's covariance="full" on the device against the
fp64 statement (tests/mixfit_full_ref.py): assign and one iteration of run on the issue's eight shapes -- and on (16453, 19, 2),
where the pass has 129 workgroups of two 64-row tiles each, so every workgroup's partial sums are read back and added to -- in five
regimes; bit-equality of two runs and of a run on a 0xFF-filled workspace; the memory contract on guarded buffers; the striped
60-iteration trajectory; the Python, model and runner surface.

Gate (the project's own): |got - ref| <= 1e-4 max(1, |ref|) per element of lse, log_resp, logw', mu', counts and the history entry;
cov' per component at 1e-4 max_de |cov'_k,de|; rows of r sum to 1 within 1e-5; cov' is bit-symmetric.  Every test prints its worst
figure before it asserts."""
import math

import numpy as np
import pytest
import torch

import mixfit_full_ref as F
import mixfit_ref as R
import mixfit_util as U
from mixfit_util import FULL, REG, cov_err, dev, gate_err, sid

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (67, 5, 3), (403, 16, 4), (1031, 64, 10), (259, 67, 3), (130, 128, 8), (2050, 2, 256), (300, 64, 256)]      # (N, L, K)
TWO_TILES = (16453, 19, 2)            # csrc/mixfit_full.hpp mff_plan: 64 rows per tile, 258 tiles, 129 workgroups of 2 tiles
ALL_SHAPES = SHAPES + [TWO_TILES]
REGIMES = ["blob", "offset50", "far", "tight", "absent"]


def spd(rng, K, Lz, lo, hi):
    """cov_k = Q diag(s^2) Q^T rounded to fp32, s uniform in [lo, hi]: a condition number of at most (hi / lo)^2."""
    out = np.zeros((K, Lz, Lz), np.float32)
    for k in range(K):
        q, _ = np.linalg.qr(rng.normal(0, 1, (Lz, Lz)))
        out[k] = ((q * rng.uniform(lo, hi, Lz) ** 2) @ q.T).astype(np.float32)
    return out


def bad_index(Lz):
    return min(2, Lz - 1)


def make_case(shape, regime):
    """(codes [N, L], logw [K], mu [K, L], cov [K, L, L]) as fp32 arrays: mu is rows of the codes, cov = Q diag(s^2) Q^T with s in
    [0.05, 3], logw random with logw[1] = -inf where K >= 2.  offset50: cluster n mod min(K, 4) shifted by 50 k in dimension 0, mu the
    first K rows -- off the centres; far: the codes then move 4000 along dimension 0; tight: cov = 1e-6 x the construction with s in
    [0.5, 2]; absent: cov_0 = diag(1, ..., 1) with -1 at index min(2, L - 1)."""
    N, Lz, K = shape
    rng = np.random.default_rng(7000 + 1000 * ALL_SHAPES.index(shape) + REGIMES.index(regime))
    z = rng.normal(0, 1, (N, Lz))
    lab = np.arange(N) % min(K, 4)
    if regime == "offset50":
        z[:, 0] += 50.0 * lab
    z = z.astype(np.float32)
    rows = np.arange(K) % N if regime == "offset50" else rng.integers(0, N, K)
    mu = z[rows].copy()
    cov = (np.float32(1e-6) * spd(rng, K, Lz, 0.5, 2.0)).astype(np.float32) if regime == "tight" else spd(rng, K, Lz, 0.05, 3.0)
    logw = rng.normal(0, 1, K)
    logw = (logw - np.log(np.exp(logw).sum())).astype(np.float32)
    if K >= 2:
        logw[1] = -np.inf
    if regime == "far":
        z[:, 0] += np.float32(4000.0)
    if regime == "absent":
        d = np.ones(Lz, np.float32)
        d[bad_index(Lz)] = -1.0
        cov[0] = np.diag(d)
    return z, logw, mu, cov


def reference(shape, regime):
    return U.reference(FULL, make_case, shape, regime)


def run_once(z, logw, mu, cov, n_iter=1):
    return U.run_once(FULL, z, logw, mu, cov, n_iter)


CASES = [(s, r) for s in ALL_SHAPES for r in REGIMES]


@pytest.mark.parametrize("shape,regime", CASES, ids=lambda v: sid(v) if isinstance(v, tuple) else v)
def test_assign_and_one_iteration_match_the_statement(shape, regime):
    from gmvae_amd import mixfit
    N, Lz, K = shape
    z, logw, mu, cov = make_case(shape, regime)
    ref = reference(shape, regime)
    want_info = np.zeros(K, np.int32)
    if regime == "absent":
        want_info[0] = bad_index(Lz) + 1
    assert np.array_equal(ref["info"], want_info)                    # (the construction's factorisations succeed on the CPU)
    o = mixfit.assign(dev(z), (dev(logw), dev(mu), dev(cov)))
    lse, lr, info = o["lse"].cpu().numpy(), o["log_resp"].cpu().numpy(), o["info"].cpu().numpy()
    live = np.isfinite(ref["lse"])
    errs = {"lse": gate_err(lse, ref["lse"]), "log_resp": gate_err(lr, ref["log_resp"]),
            "rows_of_r": float(np.abs(np.exp(lr[live].astype(np.float64)).sum(axis=1) - 1).max()) if live.any() else 0.0}
    got = run_once(z, logw, mu, cov)
    errs.update(U.one_iteration_errs(FULL, got, ref))
    print(shape, regime, {k: f"{v:.2e}" for k, v in errs.items()}, "info", info[:4].tolist())
    rows_of_r = errs.pop("rows_of_r")
    assert info.dtype == np.int32 and np.array_equal(info, want_info) and np.array_equal(got[5], want_info)
    assert max(errs.values()) <= 1e-4, errs
    assert rows_of_r <= 1e-5              # fp32: ln of a sum of at most 256 terms rounds to 3e-7, expf to 1e-7 each
    assert np.array_equal(got[2], got[2].transpose(0, 2, 1))         # cov' is bit-symmetric
    if regime == "absent":
        assert np.isneginf(lr[:, 0]).all()
        w2, m2, c2, hist, counts, info2 = run_once(z, logw, mu, cov, n_iter=2)
        assert all(np.isfinite(a).all() for a in (w2, m2, c2, counts)) and np.array_equal(info2, want_info)
    if regime == "blob":
        # cov = diag(sigma^2): lse is gmvae_mixfit_assign's, on the device
        sigma = np.random.default_rng(5).uniform(0.05, 3.0, (K, Lz)).astype(np.float32)
        dcov = np.stack([np.diag(s.astype(np.float64) ** 2) for s in sigma]).astype(np.float32)
        sig = np.sqrt(np.stack([np.diagonal(c) for c in dcov]).astype(np.float64)).astype(np.float32)
        a = mixfit.assign(dev(z), (dev(logw), dev(mu), dev(dcov)))
        b = mixfit.assign(dev(z), (dev(logw), dev(mu), dev(sig)))
        e = gate_err(a["lse"].cpu().numpy(), b["lse"].cpu().numpy())
        print(shape, "diagonal cov against gmvae_mixfit_assign:", f"{e:.2e}")
        assert e <= 1e-4 and not a["info"].any().item()


def test_two_runs_give_the_same_bits_on_any_workspace():
    U.check_same_bits_on_any_workspace(FULL, make_case, (((1031, 64, 10), "blob"), ((259, 67, 3), "offset50"), (TWO_TILES, "blob")))


def test_memory_contract_on_guarded_buffers():
    """N = 259, L = 67, K = 3.  The statement of the contract is mixfit_util's."""
    U.check_memory_contract(FULL, make_case, (259, 67, 3), 8 << 20)


# ------------------------------------------------------------------------------------------------------------ a trajectory
STRIPES = dict(N=402, L=5, K=3, seed=7, gap=8, length=8)


def stripes_case():
    z, lab = F.stripes(**STRIPES)
    logw, mu, cov = F.start(z, R.first_of_each(lab, 3))
    return z, lab, logw.astype(np.float32), mu.astype(np.float32), cov.astype(np.float32)


def trajectory_errs(got, ref):
    return dict(logw=gate_err(got["logw"], ref["logw"]), mu=gate_err(got["mu"], ref["mu"]), cov=cov_err(got["cov"], ref["cov"]))


def test_the_striped_trajectory_of_sixty_iterations():
    """Three parallel elongated clusters, 402 codes in 5 dimensions, 60 iterations from one code per cluster and cov = diag(sd^2):
    logw, mu, cov, counts and the history inside the gate of the fp64 statement's, the history never falling by more than the gate,
    every label recovered by the device's log_resp.  The fp32 statement's own deviation is printed next to the device's as the
    yardstick (measured on the CPU: 4.3e-7; the device's figure is in profiles/mixfit_full_notes.md)."""
    from gmvae_amd import mixfit
    z, lab, logw, mu, cov = stripes_case()
    ref = F.fit(z, logw, mu, cov, 60)
    f32 = F.fit(z, logw, mu, cov, 60, dtype=np.float32)
    o = mixfit.fit(dev(z), 3, n_iter=60, init=(dev(logw), dev(mu), dev(cov)), covariance="full")
    got = {k: o[k].cpu().numpy() for k in ("logw", "mu", "cov", "counts", "loglik_history", "info")}
    errs = trajectory_errs(got, ref)
    yard = trajectory_errs(f32, ref)
    herr, cerr = gate_err(got["loglik_history"], ref["loglik_history"]), gate_err(got["counts"], ref["counts"])
    dip = float(np.diff(np.append(got["loglik_history"], o["loglik"].item())).min())
    acc = R.cluster_acc(mixfit.assign(dev(z), o)["log_resp"].cpu().numpy(), lab)
    print(f"fp32 statement {max(yard.values()):.2e}; device {max(errs.values()):.2e} {errs}; history {herr:.2e}; counts {cerr:.2e}; "
          f"largest fall {min(dip, 0.0):.2e}; loglik {o['loglik'].item():.6f} (ref {ref['loglik']:.6f}); accuracy {acc}")
    assert o["centres"] is None and max(errs.values()) <= 1e-4 and herr <= 1e-4 and cerr <= 1e-4
    assert gate_err(o["loglik"].item(), ref["loglik"]) <= 1e-4 and not got["info"].any()
    assert dip >= -1e-4 * max(1.0, abs(ref["loglik"])) and acc == 1.0 and R.cluster_acc(ref["log_resp"], lab) == 1.0


# ------------------------------------------------------------------------------------------------------------------ surface
FULL_KEYS = {"logw", "mu", "cov", "counts", "loglik", "loglik_history", "centres", "info"}
DIAG_KEYS = {"logw", "mu", "sigma", "counts", "loglik", "loglik_history", "centres"}


def test_fit_full_from_the_seeding_and_several_inits():
    from gmvae_amd import mixfit
    z = R.blobs(403, 16, 4, 453)[0]
    zd = dev(z)
    singles = [mixfit.fit(zd, 4, n_iter=15, seed=s, covariance="full") for s in (5, 6, 7)]
    again = mixfit.fit(zd, 4, n_iter=15, seed=5, covariance="full")
    assert set(again) == FULL_KEYS and again["info"].dtype == torch.int32 and again["cov"].shape == (4, 16, 16)
    for k in FULL_KEYS:
        assert torch.equal(singles[0][k], again[k]), k                                  # the same seed, the same bits
    # the same seeding as the diagonal fit; the start is the statement's: the chosen rows, diag(var) of all codes, equal weights
    d0 = mixfit.fit(zd, 4, n_iter=0, seed=5)
    o0 = mixfit.fit(zd, 4, n_iter=0, seed=5, covariance="full")
    assert set(d0) == DIAG_KEYS and torch.equal(d0["centres"], o0["centres"]) and torch.equal(d0["mu"], o0["mu"]) and torch.equal(d0["logw"], o0["logw"])
    lw, mu, cov = F.start(z, o0["centres"].cpu().numpy())
    assert np.array_equal(o0["mu"].cpu().numpy(), mu.astype(np.float32)) and np.allclose(o0["cov"].cpu().numpy(), cov, rtol=1e-6, atol=0)
    assert o0["loglik_history"].shape == (0,) and not o0["info"].any().item() and abs(o0["counts"].sum().item() - 403) < 1e-2
    e = gate_err(o0["loglik"].item(), d0["loglik"].item())
    print("the first E-step against the diagonal fit's:", f"{e:.2e}")
    assert e <= 1e-4
    best = mixfit.fit(zd, 4, n_iter=15, n_init=3, seed=5, covariance="full")
    ll = [s["loglik"].item() for s in singles]
    j = int(np.argmax(ll))
    print("loglik of seeds 5, 6, 7:", ll, "-> n_init = 3 returns", best["loglik"].item())
    for k in FULL_KEYS:
        assert torch.equal(best[k], singles[j][k]), k
    eye = torch.eye(16).expand(4, 16, 16)
    for bad in (dict(K=4, covariance="tied"), dict(K=4, n_iter=-1), dict(K=4, reg_covar=0.0),
                dict(K=4, init=(torch.zeros(3), torch.zeros(3, 16), eye[:3])),                      # K = 3 components for K = 4
                dict(K=4, init=(torch.zeros(4), torch.zeros(4, 16), torch.ones(4, 16, 15))),        # a cov of the wrong shape
                dict(K=4, init=(torch.zeros(4), torch.zeros(4, 16), torch.ones(4, 16))),            # a diagonal init
                dict(K=4, n_init=2, init=(torch.zeros(4), torch.zeros(4, 16), eye))):
        with pytest.raises(ValueError):
            mixfit.fit(zd, covariance=bad.pop("covariance", "full"), **bad)
    with pytest.raises(ValueError):
        mixfit.fit(torch.zeros(8, 129), 1, covariance="full")                           # L = 129
    with pytest.raises(ValueError):
        mixfit.fit(torch.zeros(300, 64), 257, covariance="full")                        # K = 257
    with pytest.raises(ValueError):
        mixfit.fit(torch.zeros(300, 65), 256, covariance="full")                        # K L^2 = 1,081,600
    with pytest.raises(ValueError):
        mixfit.assign(zd, (torch.zeros(4), torch.zeros(4, 16), torch.ones(4, 15, 15)))
    mixfit.fit(torch.zeros(8, 129), 1, n_iter=1)                                        # (the diagonal fit takes L = 129)


def test_bic_matches_the_statement_for_both_covariances():
    from gmvae_amd import mixfit
    z, lab, logw, mu, cov = stripes_case()
    N, Lz, K = z.shape[0], z.shape[1], 3
    sigma = np.sqrt(np.stack([np.diagonal(c) for c in cov]).astype(np.float64)).astype(np.float32)
    ref_f = F.fit(z, logw, mu, cov, 20)
    ref_d = R.fit(z, logw, mu, sigma, 20)
    o_f = mixfit.fit(dev(z), K, n_iter=20, init=(dev(logw), dev(mu), dev(cov)), covariance="full")
    o_d = mixfit.fit(dev(z), K, n_iter=20, init=(dev(logw), dev(mu), dev(sigma)))
    for name, o, ref, p in (("full", o_f, ref_f, 3 - 1 + 15 + 3 * 15), ("diag", o_d, ref_d, 3 - 1 + 15 + 15)):
        assert mixfit.n_parameters(K, Lz, name) == p == F.n_parameters(K, Lz, name)
        want_b, want_a = -2 * N * ref["loglik"] + p * math.log(N), -2 * N * ref["loglik"] + 2 * p
        b, a = mixfit.bic(o, N), mixfit.aic(o, N)
        print(name, f"bic {b.item():.4f} (statement {want_b:.4f}), aic {a.item():.4f} (statement {want_a:.4f})")
        assert b.dtype == torch.float64 and gate_err(b.item(), want_b) <= 1e-4 and gate_err(a.item(), want_a) <= 1e-4
    assert mixfit.bic(o_f, N).item() < mixfit.bic(o_d, N).item()                         # the striped case prefers full covariances


def test_models_fit_full_and_refuse_it_as_a_prior():
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    x = torch.from_numpy((np.random.default_rng(2).random((96, 64)) < 0.5).astype(np.uint8)).cuda()
    plain = create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)
    gmp = create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)
    gm = create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)
    for name, model, kw in (("vae", plain, dict(n_components=3)), ("vae_gmp", gmp, {}), ("gmvae", gm, {})):
        o = model.fit_latent_mixture(x, n_iter=10, covariance="full", **kw)
        assert set(o) == FULL_KEYS | {"log_resp"}, name
        assert o["logw"].shape == (3,) and o["mu"].shape == (3, 4) and o["cov"].shape == (3, 4, 4) and o["log_resp"].shape == (96, 3)
        assert o["loglik_history"].shape == (10,) and o["centres"].shape == (3,) and o["counts"].shape == (3,) and o["info"].shape == (3,)
        assert all(torch.isfinite(o[k].double()).all() for k in FULL_KEYS), name
        assert torch.equal(o["cov"], o["cov"].transpose(1, 2))
        assert not torch.isnan(o["log_resp"]).any() and abs(o["counts"].sum().item() - 96) < 1e-2
        d = model.fit_latent_mixture(x, n_iter=10, **kw)
        assert set(d) == DIAG_KEYS | {"log_resp"}, name                                  # the default is unchanged
        if model is not plain:
            with pytest.raises(ValueError, match="diagonal"):
                model.init_prior_from_mixture(o)
            model.init_prior_from_mixture(d)


def test_run_eval_fits_the_full_mixture_and_reports_the_bic(tmp_path):
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200", "--batch_size=40"]
    run_gmvae.main(["--mode=train"] + args)
    fit_args = ["--mode=eval", "--fit_latent_mixture=64", "--mixture_fit_iters=20"]
    res = run_gmvae.main(fit_args + ["--mixture_covariance=full", "--mixture_bic"] + args)
    three = {"train/latent_mixture_loglik", "train/cluster_acc_latent_mixture", "latent_mixture"}
    four = three | {"train/latent_mixture_bic"}
    assert four <= set(res) and math.isfinite(res["train/latent_mixture_loglik"]) and math.isfinite(res["train/latent_mixture_bic"])
    assert 0.0 <= res["train/cluster_acc_latent_mixture"] <= 1.0
    fm = res["latent_mixture"]
    assert set(fm) == FULL_KEYS and fm["cov"].shape == (10, 8, 8) and fm["info"].shape == (10,) and torch.isfinite(fm["cov"]).all()
    from gmvae_amd import mixfit
    assert res["train/latent_mixture_bic"] == pytest.approx(-2 * 64 * fm["loglik"].item() + mixfit.n_parameters(10, 8, "full") * math.log(64))
    plain = run_gmvae.main(["--mode=eval"] + args)
    assert set(plain) == set(res) - four
    default = run_gmvae.main(fit_args + args)                                               # exactly today's keys
    assert set(default) == set(plain) | three and set(default["latent_mixture"]) == DIAG_KEYS
    with_bic = run_gmvae.main(fit_args + ["--mixture_bic"] + args)
    assert set(with_bic) == set(plain) | four
    assert with_bic["train/latent_mixture_bic"] == pytest.approx(
        -2 * 64 * with_bic["latent_mixture"]["loglik"].item() + mixfit.n_parameters(10, 8, "diag") * math.log(64))
    ns = run_gmvae.main(fit_args + ["--mixture_covariance=full", "--neighbour_scores=100", "--knn_k=5"] + args)
    assert all(math.isfinite(ns[f"train/{k}_latent_mixture"]) for k in ("silhouette", "nmi", "ari"))
