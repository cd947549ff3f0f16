"""gmvae_mmd (include/gmvae_hip.h; csrc/twosample.hpp) and gmvae_amd.twosample on the device against the fp64 statement
(tests/twosample_ref.py) on the shapes of tests/twosample_cases.py under both kernels and one and three bandwidths; duplicated
rows under the energy kernel; bit-equality of two runs and of a subset of the splits; stream order; the bandwidths; the test's
verdict on two pairs of Gaussian samples; the Python, model and runner surface.

Gate: mmd2, row_all / N and row_first / N within 1e-9 kscale of the statement (kscale = 1 for rbf, the root-mean-square pairwise
distance for energy): summation order in fp64 sits five orders of magnitude below it (tests/test_twosample_cpu.py), the smallest
fp32 slip -- an expf at 6e-8 -- sixty times above.  NaN exactly where the statement has it.  The count of splits at or above the
observed one equals the statement's, the splits within 2e-9 kscale of the threshold left out -- at most 1 % of them, and the cases
are chosen so that there are none.  Every test prints its worst figure before it asserts."""
import math

import numpy as np
import pytest
import torch

import twosample_cases as K
import twosample_ref as R

pytestmark = pytest.mark.gpu


def gate(name, got, ref, scale):
    """The worst |got - ref| in units of the gate, 1e-9 scale; printed, then asserted <= 1.  NaN exactly where the reference has it."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), name
    keep = ~np.isnan(ref)
    err = np.abs(got[keep] - ref[keep]).max() if keep.any() else 0.0
    print(f"  {name}: max |got - ref| = {err:.3e} = {err / (R.GATE * scale):.3e} of the gate")
    assert err <= R.GATE * scale, (name, err, scale)


def check(got, ref, N):
    """(mmd2, row_all, row_first) of the device against the reference's (.., kscale): the gate, then the exceedance count."""
    mmd2, row_all, row_first = (t.cpu().numpy() for t in got)
    scale = ref[3]
    gate("mmd2", mmd2, ref[0], scale)
    gate("row_all / N", row_all / N, ref[1] / N, scale)
    gate("row_first / N", row_first / N, ref[2] / N, scale)
    count, undecided = R.exceedances(ref[0], scale)
    print(f"  p-value: {int(undecided.sum())} of {len(undecided)} splits left out, {count} at or above the observed one")
    assert undecided.sum() <= 0.01 * len(undecided)
    with np.errstate(invalid="ignore"):
        hit = (mmd2[1:] >= mmd2[0] - R.TOL * scale) & ~undecided
    assert int(hit.sum()) == count


def check_p_value(t, ref_mmd2, scale):
    """mmd_test's dict against the statement's mmd2 [P]: the exceedance count over the decided splits (at most 1 % undecided), and
    the p-value itself where none is undecided."""
    count, undecided = R.exceedances(ref_mmd2, scale)
    assert undecided.sum() <= 0.01 * len(undecided)
    null, obs = t["null"].cpu().numpy(), t["mmd2"].item()
    with np.errstate(invalid="ignore"):
        hit = (null >= obs - R.TOL * scale) & ~undecided
    assert int(hit.sum()) == count
    if not undecided.any():
        assert t["p_value"].item() == R.p_value(ref_mmd2, scale)


@pytest.mark.parametrize("variant", K.VARIANTS, ids=K.vid)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_matches_the_statement(shape, variant):
    from gmvae_amd import twosample
    kernel, Q = variant
    z, E = K.data(shape), K.splits(shape)
    print(f"{shape} {kernel} Q = {Q}:")
    got = twosample.mmd(z, E, kernel, K.gamma(shape, Q))
    check(got, K.reference(shape, variant), z.shape[0])


def test_equal_rows_give_exactly_zero_under_the_energy_kernel():
    """Two points a sample, D = 785, rows near 1000: the first sample is {a, a}, the second {a, b}.  Every pair of equal rows has
    exactly k = 0, so row_first = K0 e_0 is exactly 0 in rows 0, 1 and 2; the expanded square would leave rounding of 1000^2 there."""
    from gmvae_amd import twosample
    rng = np.random.default_rng(7)
    a, b = (1000.0 + rng.standard_normal((2, 785))).astype(np.float32)
    z = np.stack([a, a, a, b])
    E = np.array([[1, 1, 0, 0]], dtype=np.uint8)
    mmd2, row_all, row_first = twosample.mmd(z, E, "energy")
    ref = R.mmd(z, E, "energy")
    print(f"row_first = {row_first.tolist()}, row_all = {row_all.tolist()}")
    assert row_first[:3].tolist() == [0.0, 0.0, 0.0] and row_first[3].item() < -1.0
    d = -math.sqrt(float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum()))
    assert abs(row_all[0].item() - d) <= 1e-12 * abs(d) and abs(row_first[3].item() - 2 * d) <= 1e-12 * abs(d)
    check((mmd2, row_all, row_first), ref + (R.kscale(z, "energy"),), 4)
    # and the duplicated rows of the pixel case: the kernel entry of each pair, read off a split that holds one of the two alone
    zp = K.data(K.PIXELS)
    N = zp.shape[0]
    for i, j in K.DUPLICATES:
        pair = zp[[i, i, j, j]]
        got = twosample.mmd(pair, E, "energy")
        assert not got[1].any().item() and not got[2].any().item(), (i, j)


def test_two_runs_and_a_subset_of_the_splits_give_the_same_bits():
    from gmvae_amd import twosample
    for shape in (K.OFFSET, (700, 837, 8, 64)):
        z, E = torch.from_numpy(K.data(shape)).cuda(), torch.from_numpy(K.splits(shape)).cuda()
        for kernel in ("rbf", "energy"):
            g = K.gamma(shape, 3)
            a, b = twosample.mmd(z, E, kernel, g), twosample.mmd(z, E, kernel, g)
            for s, t in zip(a, b):
                assert torch.equal(s.view(torch.int64), t.view(torch.int64)), (shape, kernel)
            few = twosample.mmd(z, E[:5], kernel, g)                      # rows 0 .. 4 alone: another chunk size, the same bits
            assert torch.equal(few[0].view(torch.int64), a[0][:5].view(torch.int64)), (shape, kernel)
            assert torch.equal(few[1].view(torch.int64), a[1].view(torch.int64)) and torch.equal(few[2].view(torch.int64), a[2].view(torch.int64))
            one = twosample.mmd(z, E[:1], kernel, g, rows=False)
            assert one[1] is None and one[2] is None and torch.equal(one[0].view(torch.int64), a[0][:1].view(torch.int64))


def test_follows_the_stream():
    """The pooled rows come out of a torch op enqueued on the same side stream just before; the result is the one of rows that
    were ready long before."""
    from gmvae_amd import twosample
    shape = (700, 837, 8, 64)
    z, E = torch.from_numpy(K.data(shape)).cuda(), torch.from_numpy(K.splits(shape)).cuda()
    g = K.gamma(shape, 3)
    ready = twosample.mmd(z, E, "rbf", g)
    half = (z * 0.5).contiguous()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            big = big @ big * 1e-3                                     # work in front of it on the stream
        zz = half + half                                               # exactly z
        got = twosample.mmd(zz, E, "rbf", g)
    side.synchronize()
    for s, t in zip(ready, got):
        assert torch.equal(s.view(torch.int64), t.view(torch.int64))
    check(got, K.reference(shape, ("rbf", 3)), z.shape[0])


def test_bandwidths_match_numpy():
    from gmvae_amd import twosample
    rng = np.random.default_rng(11)
    for N, D in ((331, 784), (2500, 3), (1024, 8), (1025, 8)):
        z = (rng.standard_normal((N, D)) * 3.0 + 5.0).astype(np.float32)
        zd = torch.from_numpy(z).cuda()
        med, mean = twosample.median_distance(zd).item(), twosample.rms_distance(zd).item()
        rmed, rmean = R.median_distance(z), R.kscale(z, "energy")
        print(f"[{N}, {D}]: median {med:.12e} (ref {rmed:.12e}), mean {mean:.12e} (ref {rmean:.12e})")
        assert abs(med - rmed) <= 1e-9 * rmed and abs(mean - rmean) <= 1e-9 * rmean
    x, y = zd[:500], zd[500:]
    for bw, sigma in (("median", rmed), ("mean", rmean), (2.5, 2.5)):
        out = twosample.mmd_test(x, y, n_perms=3, bandwidth=bw)
        assert abs(out["sigma"] - sigma) <= 1e-9 * sigma
        ref = R.mmd(z, twosample.permutations(500, 525, 3, 0).numpy(), "rbf", R.gammas(out["sigma"]))
        gate(f"mmd2 at bandwidth={bw!r}", torch.cat([out["mmd2"][None], out["null"]]).cpu().numpy(), ref[0], 1.0)
    out = twosample.mmd_test(x, y, n_perms=2, bandwidth=[1.0, 4.0])
    assert out["sigma"] == [1.0, 4.0]
    gate("mmd2 at two given bandwidths", out["mmd2"].item(), R.mmd(z, twosample.permutations(500, 525, 1, 0).numpy(), "rbf", [0.5, 1 / 32])[0][0], 1.0)


def test_verdicts_on_gaussian_samples():
    """N(0, I) against N(0.5, I) at n = m = 256, D = 8, P = 200: no permutation reaches the observed statistic, p = 1 / 200.  Two
    samples of N(0, I): the p-value is the statement's, and so are the witness function and the null."""
    from gmvae_amd import twosample
    rng = np.random.default_rng(21)
    x = rng.standard_normal((256, 8)).astype(np.float32)
    y = (0.5 + rng.standard_normal((256, 8))).astype(np.float32)
    w = rng.standard_normal((256, 8)).astype(np.float32)
    for kernel in ("rbf", "energy"):
        out = twosample.mmd_test(x, y, n_perms=200, kernel=kernel, seed=3)
        print(f"{kernel}: shifted mmd2 = {out['mmd2'].item():.6e}, p = {out['p_value'].item()}")
        assert out["p_value"].item() == 1 / 200 and out["n_perms"] == 200 and out["null"].shape == (199,)
        assert out["witness_x"].shape == (256,) and out["witness_y"].shape == (256,)
        assert out["witness_x"].mean().item() > 0 > out["witness_y"].mean().item()
        same = twosample.mmd_test(x, w, n_perms=200, kernel=kernel, seed=3)
        z, E = np.concatenate([x, w]), twosample.permutations(256, 256, 200, 3).numpy()
        scale = R.kscale(z, kernel)
        ref = R.mmd(z, E, kernel, R.gammas(same["sigma"]) if kernel == "rbf" else ())
        _, undecided = R.exceedances(ref[0], scale)
        print(f"{kernel}: same mmd2 = {same['mmd2'].item():.6e}, p = {same['p_value'].item()}, ref p = {R.p_value(ref[0], scale)}")
        assert not undecided.any() and same["p_value"].item() == R.p_value(ref[0], scale)
        assert abs(same["kscale"].item() - scale) <= 1e-9 * scale
        gate("null", same["null"].cpu().numpy(), ref[0][1:], scale)
        wit = R.witness(ref[1], ref[2], E[0])
        # (row_first / (N / 2) and (row_all - row_first) / (N / 2), each row sum over N within one gate: two gates and four)
        gate("witness", torch.cat([same["witness_x"], same["witness_y"]]).cpu().numpy(), wit, 6.0 * scale)
    # the splits given: mmd_test with assignments= is mmd on them; mmd2() is the observed split alone
    E = twosample.permutations(256, 256, 7, 5)
    given = twosample.mmd_test(x, y, kernel="energy", assignments=E)
    direct = twosample.mmd(np.concatenate([x, y]), E, "energy")[0]
    assert given["n_perms"] == 7 and torch.equal(torch.cat([given["mmd2"][None], given["null"]]), direct)
    alone = twosample.mmd2(x, y, kernel="energy")
    assert torch.equal(alone["mmd2"], direct[0]) and alone["p_value"].item() == 1.0 and alone["null"].shape == (0,)


def test_models_test_their_samples():
    """model.sample_test on a small VAE, mixture-prior VAE and GMVAE: "data" is mmd_test of simulate's x against the images, "code"
    of simulate's z against one draw of q(z | x) (the GMVAE's transform; the VAE's encoder(x).sample(), not its mean)."""
    from gmvae_amd import twosample
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(3)
    x = torch.from_numpy((rng.random((96, 64)) < 0.5).astype(np.uint8)).cuda()
    for name, model in (("vae", create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)),
                        ("vae_gmp", create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)),
                        ("gmvae", create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1))):
        both = model.sample_test(x, space="both", n_perms=50, seed=2)
        assert set(both) == {"data", "code"}, name
        sim = model.simulate(96)
        code = model.transform(x) if name == "gmvae" else model.encoder(x).sample(seed=model.random_seed)
        E = twosample.permutations(96, 96, 50, 2).numpy()
        for space, (a, b) in (("data", (sim["x"].float(), x.float())), ("code", (sim["z"], code))):
            t = both[space]
            z = torch.cat([a, b]).cpu().numpy()
            ref = R.mmd(z, E, "rbf", R.gammas(t["sigma"]))
            print(f"{name} {space}: mmd2 = {t['mmd2'].item():.6e}, p = {t['p_value'].item()}, sigma = {t['sigma']:.6f}")
            assert abs(t["sigma"] - R.median_distance(z)) <= 1e-9 * t["sigma"]
            gate("mmd2 and null", torch.cat([t["mmd2"][None], t["null"]]).cpu().numpy(), ref[0], 1.0)
            check_p_value(t, ref[0], 1.0)
        if name != "gmvae":
            assert not torch.equal(code, model.transform(x))                 # a draw, not the mean
        only = model.sample_test(x, n_generations=40, space="code", n_perms=5, kernel="energy")
        assert set(only) == {"code"} and only["code"]["witness_x"].shape == (40,) and only["code"]["witness_y"].shape == (96,)
        assert set(model.sample_test(x, n_perms=2)) == {"data"}
        with pytest.raises(ValueError):
            model.sample_test(x, space="pixels")
    grey = create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1, likelihood="continuous_bernoulli")
    with pytest.raises(ValueError, match="simulate"):
        grey.sample_test(x, space="data", n_perms=2)
    assert twosample.workspace_bytes(192, 64, 50) > 0


def _corr(a, b):
    a, b = a.double().flatten() - a.double().mean(), b.double().flatten() - b.double().mean()
    return (a @ b / (a.norm() * b.norm())).item()


@pytest.mark.parametrize("likelihood", ["continuous_bernoulli", "gaussian"])
def test_code_space_under_a_likelihood_simulate_refuses(likelihood):
    """Grey-level models (no simulate): space="code" draws the prior itself, on a stream independent of the posterior draw.  Every
    sample(seed=s) starts a fresh generator at s, so a prior drawn with the model's own seed -- generate_samples -- consumes the
    posterior draw's normal numbers: for the plain VAE it IS that noise.  Held here: the test's result is the statement's on
    (_prior_draws, the posterior draw); the prior draws are not generate_samples'; and their correlation with the posterior draw's
    noise eps = (code - mu) / sigma is that of independent numbers: 96 * 4 pairs, standard deviation 0.051, bound 0.25."""
    from gmvae_amd import twosample
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(0, 256, (96, 64)).astype(np.uint8)).cuda()
    E = twosample.permutations(96, 96, 50, 2).numpy()
    for name, model in (("vae", create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1, likelihood=likelihood)),
                        ("vae_gmp", create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1, likelihood=likelihood)),
                        ("gmvae", create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1, likelihood=likelihood))):
        with pytest.raises(ValueError, match="simulate"):
            model.sample_test(x, space="both", n_perms=2)
        t = model.sample_test(x, space="code", n_perms=50, seed=2)["code"]
        if name == "gmvae":
            code = model.transform(x)
            q = model.encoder_gmm(x, model.encoder_y(x).sample(seed=model.random_seed))
        else:
            q = model.encoder(x)
            code = q.sample(seed=model.random_seed)
        prior = twosample._prior_draws(model, 96)
        assert prior.shape == (96, 4) and torch.equal(prior, twosample._prior_draws(model, 96))      # seeded: the same draws again
        z = torch.cat([prior, code]).cpu().numpy()
        ref = R.mmd(z, E, "rbf", R.gammas(t["sigma"]))
        print(f"{likelihood} {name}: mmd2 = {t['mmd2'].item():.6e}, p = {t['p_value'].item()}, sigma = {t['sigma']:.6f}")
        assert abs(t["sigma"] - R.median_distance(z)) <= 1e-9 * t["sigma"]
        gate("mmd2 and null", torch.cat([t["mmd2"][None], t["null"]]).cpu().numpy(), ref[0], 1.0)
        check_p_value(t, ref[0], 1.0)
        eps = (code - q.loc) / q.scale_diag                                   # the posterior draw's noise
        coupled = model.generate_samples(96) if name != "gmvae" else None      # what the model's own seed would have drawn
        c_new = _corr(prior, eps)
        print(f"  corr(prior draws, posterior noise) = {c_new:+.3f}" + ("" if coupled is None else f"; generate_samples': {_corr(coupled, eps):+.3f}"))
        assert abs(c_new) <= 0.25
        if coupled is not None:
            assert not torch.equal(prior, coupled)
        if name == "vae":                                                     # N(0, I): the prior draw is its own noise
            assert (coupled - eps).abs().max().item() <= 1e-3 and (prior - eps).abs().max().item() > 1.0
    # a model without a seed draws from torch's global generators: two calls, two samples
    free = create_vae(64, 4, fcnet_hidden_sizes=[16], likelihood=likelihood)
    assert not torch.equal(twosample._prior_draws(free, 96), twosample._prior_draws(free, 96))


def test_no_statistic_no_p_value():
    """Split 0 with one point on a side: mmd2 is NaN, and so are the p-value (not 1 / P) and the witness function."""
    from gmvae_amd import twosample
    rng = np.random.default_rng(8)
    x, y = rng.standard_normal((1, 3)).astype(np.float32), rng.standard_normal((9, 3)).astype(np.float32)
    for kernel in ("rbf", "energy"):
        t = twosample.mmd_test(x, y, n_perms=20, kernel=kernel, bandwidth=1.0)
        assert math.isnan(t["mmd2"].item()) and math.isnan(t["p_value"].item())
        assert torch.isnan(t["witness_x"]).all().item() and torch.isnan(t["witness_y"]).all().item() and t["null"].shape == (19,)
    ok = twosample.mmd_test(np.concatenate([x, x + 1]), y, n_perms=20, bandwidth=1.0)
    assert 1 / 20 <= ok["p_value"].item() <= 1.0 and torch.isfinite(ok["witness_x"]).all().item()


def test_run_eval_reports_the_sample_test(tmp_path):
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=300", "--batch_size=50"]
    run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--sample_test=120", "--sample_test_perms=40", "--sample_test_space=both"] + args)
    for k in ("mmd2_data", "mmd_p_data", "mmd2_code", "mmd_p_code"):
        assert f"train/{k}" in res and math.isfinite(res[f"train/{k}"]), k
    for space in ("data", "code"):
        t = res["sample_test"][space]
        assert t["n_perms"] == 40 and t["null"].shape == (39,) and t["witness_x"].shape == (120,) and t["witness_y"].shape == (120,)
        assert res[f"train/mmd2_{space}"] == t["mmd2"].item() and res[f"train/mmd_p_{space}"] == t["p_value"].item()
        assert 1 / 40 <= t["p_value"].item() <= 1.0
        assert t["p_value"].item() == (1 + (t["null"] >= t["mmd2"] - 1e-8).sum().item()) / 40
    res = run_gmvae.main(["--mode=eval", "--sample_test=64", "--sample_test_perms=10", "--sample_test_kernel=energy"] + args)
    assert "train/mmd2_data" in res and "train/mmd2_code" not in res and set(res["sample_test"]) == {"data"}


def test_run_eval_tests_the_code_of_a_grey_level_model(tmp_path):
    """--sample_test_space=code under a likelihood without simulate: the prior drawn on its own stream (--random_seed is set)."""
    from gmvae_amd import run_gmvae
    args = ["--model=vae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}", "--random_seed=1",
            "--synthetic_size=300", "--batch_size=50", "--likelihood=continuous_bernoulli"]
    run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--sample_test=120", "--sample_test_perms=40", "--sample_test_space=code"] + args)
    t = res["sample_test"]["code"]
    assert set(res["sample_test"]) == {"code"} and "train/mmd2_data" not in res and math.isfinite(res["train/mmd2_code"])
    assert res["train/mmd_p_code"] == t["p_value"].item() == (1 + (t["null"] >= t["mmd2"] - 1e-8).sum().item()) / 40
    assert t["witness_x"].shape == (120,) and t["witness_y"].shape == (120,)
