"""gmvae_mixfit_* (include/gmvae_hip.h; csrc/mixfit.hpp) and gmvae_amd.mixfit on the device against the fp64 statement
(tests/mixfit_ref.py): assign and one iteration of run on the issue's seven shapes -- and on (300, 4096, 4), where a tile is one row
and every workgroup walks two tiles, so its partial sums are read back and added to -- in five regimes; bit-equality of two runs
and of a run on a NaN-filled workspace; the memory contract on guarded buffers; a 30-iteration trajectory; the seeding; the model
and runner surface.

Gate (the project's own): |got - ref| <= 1e-4 max(1, |ref|) per element of lse, log_resp, logw', mu', counts and the history entry;
sigma' relative to itself at 1e-4; in the offset regimes additionally |mu' - ref| <= 1e-3 sigma_ref beyond the rounding of the fp32
array mu' is returned in (offset_mu_err).  Every test prints its worst figure before it asserts."""
import math

import numpy as np
import pytest
import torch

import mixfit_ref as R
import mixfit_util as U
import oracle as O
from mixfit_util import DIAG, REG, _L, dev, gate_err, sid

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (67, 5, 3), (403, 16, 4), (1031, 64, 10), (259, 67, 65), (130, 128, 128), (2050, 2, 256)]      # (N, L, K)
TWO_TILES = (300, 4096, 4)            # csrc/mixfit.hpp mf_plan: 1 row per tile, 150 workgroups of 2 tiles
ALL_SHAPES = SHAPES + [TWO_TILES]
REGIMES = ["blob", "offset50", "offset1000", "far", "tight"]


def make_case(shape, regime):
    """(codes [N, L], logw [K], mu [K, L], sigma [K, L]) as fp32 arrays: mu is rows of the codes, sigma in [0.05, 3], logw random
    with one -inf entry where K >= 2.  offset50 / offset1000: cluster k = n mod min(K, 4) shifted by 50 k / 1000 k in dimension 0, mu
    the first K rows, so every cluster holds components; far: the codes then move 4000 along dimension 0, at least 1e3 sigma from every component; tight: sigma = 1e-3."""
    N, Lz, K = shape
    rng = np.random.default_rng(1000 * ALL_SHAPES.index(shape) + REGIMES.index(regime))
    z = rng.normal(0, 1, (N, Lz))
    lab = np.arange(N) % min(K, 4)                 # four clusters, as in the trajectory below and in tests/test_tsne.py
    if regime.startswith("offset"):
        z[:, 0] += float(regime[6:]) * lab
    z = z.astype(np.float32)
    rows = np.arange(K) % N if regime.startswith("offset") else rng.integers(0, N, K)
    mu = z[rows].copy()
    sigma = (np.full((K, Lz), 1e-3) if regime == "tight" else rng.uniform(0.05, 3.0, (K, Lz))).astype(np.float32)
    logw = rng.normal(0, 1, K)
    logw = (logw - np.log(np.exp(logw).sum())).astype(np.float32)
    if K >= 2:
        logw[1] = -np.inf
    if regime == "far":
        z[:, 0] += np.float32(4000.0)
    return z, logw, mu, sigma


def reference(shape, regime):
    return U.reference(DIAG, make_case, shape, regime)


def device_lse_by_mixture_logpdf(z, logw, mu, sigma):
    """ln p(z_n) of the same mixture from gmvae_mixture_logpdf_* (one chunk of K components, no per-dimension part)."""
    import ctypes as C
    L = _L()
    N, Lz = z.shape
    nb = C.c_uint64()
    L.check(L.lib.gmvae_mixture_logpdf_workspace_bytes(N, Lz, 0, C.byref(nb)), "size")
    ws = torch.zeros(nb.value // 8, dtype=torch.float64, device="cuda")
    zd, md, sd, wd = dev(z), dev(mu), dev(sigma), dev(logw)
    out = torch.empty(N, dtype=torch.float32, device="cuda")
    L.check(L.lib.gmvae_mixture_logpdf_accumulate(L.ptr(zd), N, Lz, L.ptr(md), L.ptr(sd), L.ptr(wd), mu.shape[0], 0, 1, None, 0,
                                                  L.ptr(ws), L.current_stream()), "accumulate")
    L.check(L.lib.gmvae_mixture_logpdf_finish(N, Lz, 0, 0.0, L.ptr(out), None, None, L.ptr(ws), L.current_stream()), "finish")
    return out.cpu().numpy()


def offset_mu_err(mu_got, ref):
    """max (|mu' - ref| - 2^-24 |ref|) / sigma_ref, floored at 0: the offset regimes' extra check.  The 2^-24 |ref| is the rounding of
    the fp32 array the ABI returns mu' in, which no implementation can go below: at |mu| = 3000 it is 1.8e-4, and against the
    sigma' of a component that holds two near points (N = 130, K = 128) the fp64 statement ROUNDED TO FP32 is already 6.7e-3
    sigma_ref from itself (1.0e-3 at N = 259, K = 65; measured on the CPU).  Whatever exceeds that rounding is the kernel's."""
    excess = np.abs(mu_got.astype(np.float64) - ref["mu"]) - 2.0 ** -24 * np.abs(ref["mu"])
    return float((np.maximum(excess, 0.0) / ref["sigma"]).max())


CASES = [(s, r) for s in ALL_SHAPES for r in REGIMES if not (s == TWO_TILES and r in ("offset1000", "tight"))]


@pytest.mark.parametrize("shape,regime", CASES, ids=lambda v: sid(v) if isinstance(v, tuple) else v)
def test_assign_and_one_iteration_match_the_statement(shape, regime):
    from gmvae_amd import mixfit
    z, logw, mu, sigma = make_case(shape, regime)
    ref = reference(shape, regime)
    # (the statement's own rows of r sum to 1 up to the fp64 rounding of lse, which is 1.5e-8 where l is 1e8: the tight regime)
    assert np.isfinite(ref["lse"]).all()
    assert np.abs(np.exp(ref["log_resp"]).sum(axis=1) - 1).max() < 1e-12 + 8 * np.finfo(np.float64).eps * np.abs(ref["lse"]).max()
    if regime == "far":
        assert (np.abs(z[:, None, 0] - mu[None, :, 0]) / sigma[None, :, 0]).min() >= 1e3
    o = mixfit.assign(dev(z), (dev(logw), dev(mu), dev(sigma)))
    lse, lr = o["lse"].cpu().numpy(), o["log_resp"].cpu().numpy()
    errs = {"lse": gate_err(lse, ref["lse"]), "log_resp": gate_err(lr, ref["log_resp"]),
            "rows_of_r": float(np.abs(np.exp(lr.astype(np.float64)).sum(axis=1) - 1).max()),
            "lse_vs_mixture_logpdf": gate_err(lse, device_lse_by_mixture_logpdf(z, logw, mu, sigma))}
    got = U.run_once(DIAG, z, logw, mu, sigma)
    mu2 = got[1]
    errs.update(U.one_iteration_errs(DIAG, got, ref))
    mu_in_sigma = offset_mu_err(mu2, ref)
    raw = float((np.abs(mu2 - ref["mu"]) / ref["sigma"]).max())
    print(shape, regime, {k: f"{v:.2e}" for k, v in errs.items()}, f"|mu' - ref| / sigma_ref {raw:.2e}, beyond the fp32 output's rounding {mu_in_sigma:.2e}")
    rows_of_r = errs.pop("rows_of_r")
    assert max(errs.values()) <= 1e-4, errs
    assert rows_of_r <= 1e-5              # fp32: ln of a sum of at most 256 terms rounds to 3e-7, expf to 1e-7 each
    if regime.startswith("offset"):
        assert mu_in_sigma <= 1e-3


def test_two_runs_give_the_same_bits_on_any_workspace():
    U.check_same_bits_on_any_workspace(DIAG, make_case, (((1031, 64, 10), "blob"), ((259, 67, 65), "offset50"), (TWO_TILES, "blob")))


def test_memory_contract_on_guarded_buffers():
    """N = 259, L = 67, K = 65: no size is a multiple of anything.  The statement of the contract is mixfit_util's."""
    U.check_memory_contract(DIAG, make_case, (259, 67, 65), 24 << 20)


# ------------------------------------------------------------------------------------------------------------ a trajectory
# N = 400, L = 16, K = 4, clusters 50 apart in dimension 0, init: one code per cluster, unit scales, equal weights; 30 iterations.
# The statement evaluated in fp32 NumPy (mixfit_ref with dtype=float32) against its fp64 evaluation on this case, measured on the
# CPU: the worst |x - ref| / max(1, |ref|) over logw, mu and sigma (profiles/mixfit_notes.md).  The device gets 10 times that.
FP32_STATEMENT = 2.51e-7
TRAJECTORY_TOL = 10 * FP32_STATEMENT


def trajectory_case():
    z, lab = R.blobs(400, 16, 4, 400, sep=0.0, offset=50.0)
    logw, mu, sigma = R.start(z, R.first_of_each(lab, 4))
    return z, lab, logw.astype(np.float32), mu.astype(np.float32), np.ones_like(sigma, dtype=np.float32)


def trajectory_err(got, ref):
    return max(gate_err(got[k], ref[k]) for k in ("logw", "mu", "sigma"))


def test_a_trajectory_of_thirty_iterations():
    """The device after 30 iterations against the fp64 statement: logw, mu and sigma within 10 x the fp32 statement's own deviation
    (measured on the CPU: 2.51e-7, so 2.51e-6; the device's figure on the MI355X is 5.76e-8, profiles/mixfit_notes.md), the history within the gate
    of the statement's and never falling by more than the gate, every label recovered by the device's log_resp."""
    from gmvae_amd import mixfit
    z, lab, logw, mu, sigma = trajectory_case()
    ref = R.fit(z, logw, mu, sigma, 30)
    f32 = R.fit(z, logw, mu, sigma, 30, dtype=np.float32)
    measured = trajectory_err(f32, ref)
    o = mixfit.fit(dev(z), 4, n_iter=30, init=(dev(logw), dev(mu), dev(sigma)))
    got = {k: o[k].cpu().numpy() for k in ("logw", "mu", "sigma", "counts", "loglik_history")}
    err = trajectory_err(got, ref)
    herr = gate_err(got["loglik_history"], ref["loglik_history"])
    dip = float(np.diff(np.append(got["loglik_history"], o["loglik"].item())).min())
    acc = R.cluster_acc(mixfit.assign(dev(z), o)["log_resp"].cpu().numpy(), lab)
    print(f"fp32 statement {measured:.2e} (recorded {FP32_STATEMENT:.2e}); device {err:.2e} (tol {TRAJECTORY_TOL:.2e}); history {herr:.2e}; "
          f"largest fall {min(dip, 0.0):.2e}; loglik {o['loglik'].item():.6f} (ref {ref['loglik']:.6f}); accuracy {acc}")
    assert measured <= 2 * FP32_STATEMENT                       # the recorded yardstick is this case's
    assert o["centres"] is None and err <= TRAJECTORY_TOL and herr <= 1e-4
    assert gate_err(o["loglik"].item(), ref["loglik"]) <= 1e-4 and gate_err(got["counts"], ref["counts"]) <= 1e-4
    assert dip >= -1e-4 * max(1.0, abs(ref["loglik"])) and acc == 1.0 and R.cluster_acc(ref["log_resp"], lab) == 1.0


# ------------------------------------------------------------------------------------------------------------------ seeding
SEED_SHAPES = [(403, 16, 4), (1031, 64, 10)]
SEEDS = [0, 1, 2, 3]


def seeding_codes(shape):
    return R.blobs(shape[0], shape[1], shape[2], 50 + shape[0])[0]


def cpu_uniforms(K, seed):
    return O.noise(1, 1, K, 0, seed, 0)[1][0]


@pytest.mark.parametrize("shape", SEED_SHAPES, ids=sid)
def test_kmeanspp_returns_the_statement_s_indices(shape):
    from gmvae_amd import mixfit
    z = seeding_codes(shape)
    K = shape[2]
    zd = dev(z)
    seen = []
    for seed in SEEDS:
        u = cpu_uniforms(K, seed)
        assert np.array_equal(mixfit.uniforms(K, seed).cpu().numpy(), u)
        want, margin = R.kmeanspp(z, K, u)
        got = mixfit.kmeanspp(zd, K, seed)
        print(shape, "seed", seed, "margin", f"{margin:.2e}", want.tolist(), got.tolist())
        assert margin >= 1e-9                                   # (checked on the CPU when the seeds were chosen: all four qualify)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, mixfit.kmeanspp(zd, K, seed))
        seen.append(tuple(want.tolist()))
    assert len(set(seen)) == len(SEEDS)                         # another seed, other centres


def test_fit_from_the_seeding_and_several_inits():
    from gmvae_amd import mixfit
    z = seeding_codes(SEED_SHAPES[0])
    zd = dev(z)
    singles = [mixfit.fit(zd, 4, n_iter=15, seed=s) for s in (5, 6, 7)]
    again = mixfit.fit(zd, 4, n_iter=15, seed=5)
    for k in ("logw", "mu", "sigma", "counts", "loglik", "loglik_history", "centres"):
        assert torch.equal(singles[0][k], again[k]), k                                  # the same seed, the same bits
    assert not torch.equal(singles[0]["centres"], singles[1]["centres"])
    # the start is the statement's: the chosen rows, the codes' standard deviation, equal weights
    o0 = mixfit.fit(zd, 4, n_iter=0, seed=5)
    lw, mu, sg = R.start(z, o0["centres"].cpu().numpy())
    assert np.array_equal(o0["mu"].cpu().numpy(), mu.astype(np.float32)) and np.allclose(o0["sigma"].cpu().numpy(), sg, rtol=1e-6)
    assert np.allclose(o0["logw"].cpu().numpy(), lw, rtol=1e-6) and o0["loglik_history"].shape == (0,)
    best = mixfit.fit(zd, 4, n_iter=15, n_init=3, seed=5)
    ll = [s["loglik"].item() for s in singles]
    j = int(np.argmax(ll))
    print("loglik of seeds 5, 6, 7:", ll, "-> n_init = 3 returns", best["loglik"].item())
    for k in ("logw", "mu", "sigma", "counts", "loglik", "loglik_history", "centres"):
        assert torch.equal(best[k], singles[j][k]), k
    for bad in (dict(K=0), dict(K=257), dict(K=4, n_iter=-1), dict(K=4, n_init=0), dict(K=4, reg_covar=0.0), dict(K=4, reg_covar=float("nan")),
                dict(K=4, init=(torch.zeros(3), torch.zeros(3, 16), torch.ones(3, 16))),
                dict(K=4, n_init=2, init=(torch.zeros(4), torch.zeros(4, 16), torch.ones(4, 16)))):
        with pytest.raises(ValueError):
            mixfit.fit(zd, **bad)
    with pytest.raises(ValueError):
        mixfit.fit(torch.zeros(8, 2048), 9)                                             # K L = 18,432
    with pytest.raises(ValueError):
        mixfit.assign(zd, (torch.zeros(4), torch.zeros(4, 15), torch.ones(4, 15)))


# ------------------------------------------------------------------------------------------------------------------ surface
FIT_KEYS = {"logw", "mu", "sigma", "counts", "loglik", "loglik_history", "centres", "log_resp"}


def test_models_fit_and_take_the_mixture_as_their_prior():
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    import torch.nn.functional as F
    x = torch.from_numpy((np.random.default_rng(2).random((96, 64)) < 0.5).astype(np.uint8)).cuda()
    plain = create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)
    gmp = create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)
    gm = create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)
    with pytest.raises(ValueError, match="n_components"):
        plain.fit_latent_mixture(x)
    fits = {}
    for name, model, kw in (("vae", plain, dict(n_components=3)), ("vae_gmp", gmp, {}), ("gmvae", gm, {})):
        o = model.fit_latent_mixture(x, n_iter=10, **kw)
        assert set(o) == FIT_KEYS, name
        assert o["logw"].shape == (3,) and o["mu"].shape == (3, 4) == o["sigma"].shape and o["log_resp"].shape == (96, 3)
        assert o["loglik_history"].shape == (10,) and o["centres"].shape == (3,) and o["counts"].shape == (3,)
        assert all(torch.isfinite(o[k].double()).all() for k in FIT_KEYS - {"log_resp"}), name
        assert not torch.isnan(o["log_resp"]).any() and abs(o["counts"].sum().item() - 96) < 1e-2
        fits[name] = o
    with pytest.raises(ValueError, match="no mixture prior"):
        plain.init_prior_from_mixture(fits["vae"])
    wrong_k = gmp.fit_latent_mixture(x, n_components=2, n_iter=2)
    for model in (gmp, gm):
        with pytest.raises(ValueError, match="does not match"):
            model.init_prior_from_mixture(wrong_k)
        with pytest.raises(ValueError, match="does not match"):
            model.init_prior_from_mixture((torch.zeros(3), torch.zeros(3, 5), torch.ones(3, 5)))
    # VAE_GMP: the prior is the fit
    f = fits["vae_gmp"]
    step = gmp._engine.global_step
    gmp.init_prior_from_mixture(f)
    pr = gmp.prior()
    v = gmp._engine.views()
    got = {"logw": torch.log_softmax(v["mixture_logits"], dim=0), "mu": v["loc"], "sigma": F.softplus(v["raw_scale_diag"])}
    errs = {k: ((got[k] - f[k]).abs() / f[k].abs().clamp_min(1e-30)).max().item() for k in got}
    print("vae_gmp prior after init, relative:", errs)
    assert max(errs.values()) <= 1e-6 and pr is not None and gmp._engine.global_step == step
    # GMVAE: prior_gmm(e_k) = N(mu_k, max(sigma_k, sigma_min)); p(y) stays uniform
    f = fits["gmvae"]
    gm.init_prior_from_mixture(f)
    e = gm._engine
    mu, sigma = e._normal_head(e.mlp(_L().NET_PRIOR_GMM, torch.eye(3, device="cuda")))
    want = f["sigma"].clamp_min(float(e.hp["sigma_min"]))
    errs = {"mu": ((mu - f["mu"]).abs() / f["mu"].abs().clamp_min(1.0)).max().item(), "sigma": ((sigma - want).abs() / want).max().item()}
    print("gmvae prior_gmm after init:", errs)
    assert max(errs.values()) <= 2e-6
    # a training step afterwards runs and is finite
    for model in (gmp, gm):
        loss = model.run_model(x, x)
        loss.backward()
        model._engine.adam(1e-3)
        torch.cuda.synchronize()
        assert math.isfinite(loss.item()) and torch.isfinite(model.params).all()


def test_run_eval_fits_the_latent_mixture(tmp_path):
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200", "--batch_size=40"]
    run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--fit_latent_mixture=64", "--mixture_fit_iters=20"] + args)
    new = {"train/latent_mixture_loglik", "train/cluster_acc_latent_mixture", "latent_mixture"}
    assert new <= set(res) and math.isfinite(res["train/latent_mixture_loglik"])
    assert 0.0 <= res["train/cluster_acc_latent_mixture"] <= 1.0
    fm = res["latent_mixture"]
    assert fm["mu"].shape == (10, 8) and fm["loglik_history"].shape == (20,) and torch.isfinite(fm["sigma"]).all()
    plain = run_gmvae.main(["--mode=eval"] + args)
    assert set(plain) == set(res) - new and not new & set(plain)
    vae_args = [a if not a.startswith("--model") else "--model=vae" for a in args] + [f"--logdir={tmp_path}/vae"]
    run_gmvae.main(["--mode=train"] + vae_args)
    res = run_gmvae.main(["--mode=eval", "--fit_latent_mixture=200", "--mixture_fit_iters=5", "--mixture_components=5"] + vae_args)
    assert 0.0 <= res["train/cluster_acc_latent_mixture"] <= 1.0 and res["latent_mixture"]["mu"].shape == (5, 8)
