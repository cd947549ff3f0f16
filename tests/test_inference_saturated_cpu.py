"""The conditions of tests/test_inference_saturated.py's cases, without a device: asserted on the fp64 statements alone
(tests/inference_saturated_cases.py) on the restated noise, with the values printed.  A case that misses one gets another seed, T
or step0 there, with the reason in a comment; the conditions stay.  (The restated Box-Muller agrees with the device's to a few
1e-6, not to the bit, so the device test asserts the 10 % cap again on its own draws.)"""
import dataclasses

import numpy as np
import pytest

import ais_ref as A
import inference_saturated_cases as SC
import refine_ref as RF

FP32_MAX = 3.4e38
GATE = 1e-4                   # test_ais.TOL, test_refine.TOL


# ======================================================================================================================= AIS
@pytest.mark.parametrize("name", list(SC.AIS))
def test_ais_case(name):
    c, r = SC.AIS[name], SC.ais_cpu(name)
    kept, n = r["kept"], r["kept"].size
    rate = r["accepts"].mean()
    past = ~np.isfinite(r["h_new"]) | (np.abs(r["h_new"]) > FP32_MAX)
    print(f"{name}: left out {int((~kept).sum())} of {n} (undecided {int((~r['decided']).sum())}, ill-conditioned "
          f"{int((~r['well']).sum())}), accept rate {rate:.3f}, max |log w| {np.abs(r['logw']).max():.3e}, H_new not finite "
          f"{int((~np.isfinite(r['h_new'])).sum())} / past fp32 {int(past.sum())} of {past.size}, final steps "
          f"[{r['steps'].min():.3e}, {r['steps'].max():.3e}], clipped at the low / high end {r['clips'].astype(bool).sum(axis=0).tolist()}")
    for k in ("logw", "bound", "stats", "z", "tail"):                 # every output is finite: what is not finite is rejected
        assert np.isfinite(r[k]).all(), k
    assert (~kept).mean() <= SC.CAP
    if c.kind in ("parity", "inf_eps"):
        assert not (~np.isfinite(r["h_new"])).any() or c.kind == "inf_eps"
        if c.regime == "trained":
            assert 0.0 < rate < 1.0
        elif c.mname != "vae":                                         # the mixture priors' sigma of 2e-9: nothing is accepted
            assert rate == 0.0
    if c.kind == "clip_low":
        assert rate == 0.0 and np.all(r["steps"] == A.STEP_MIN) and np.all(r["clips"][:, 0] > 0)
    if c.kind == "clip_high":
        hit = r["clips"][:, 1] > 0
        assert hit.any() and (hit & kept).any() and np.all(r["steps"][hit & r["accepts"][-1]] == A.STEP_MAX)
    if c.kind == "inf_eps":
        for t, chain in c.inject:
            assert not np.isfinite(r["h_new"][t - 1, chain]) and not r["accepts"][t - 1, chain] and kept[chain]
            assert r["accepts"][t:, chain].any()                       # the chain moves on after the reject
        assert int((~np.isfinite(r["h_new"])).sum()) == len(c.inject)
        assert {chain // 16 for _, chain in c.inject} == {0, 1} and c.B * c.C % 16      # a full panel and the ragged one
    if c.kind == "overflow":
        assert past.any(axis=0).mean() > 0.5 and rate == 0.0 and kept.all()
        assert np.array_equal(r["z"], r["z0"])
        twin = SC.AIS[SC.OVERFLOW_TWIN[name]]
        assert SC._key(twin) == SC._key(c) and (twin.T, twin.C, twin.init) == (c.T, c.C, c.init)
        assert SC.ais_cpu(SC.OVERFLOW_TWIN[name])["accepts"].sum() == 0


def test_ais_the_clip_is_reached_at_each_end():
    lo = sum(int((SC.ais_cpu(n)["clips"][:, 0] > 0).sum()) for n, c in SC.AIS.items() if c.kind == "clip_low")
    hi = sum(int((SC.ais_cpu(n)["clips"][:, 1] > 0).sum()) for n, c in SC.AIS.items() if c.kind == "clip_high")
    print(f"chains clipped at kAisStepMin {lo}, at kAisStepMax {hi}")
    assert lo > 0 and hi > 0


def test_ais_an_overflow_case_is_finite_in_fp64_and_one_is_not():
    """H_new past fp32's largest number but finite in fp64 (the guard sees inf or NaN where the statement sees a number), and NaN in
    fp64 as well."""
    got = {n: SC.ais_cpu(n)["h_new"] for n, c in SC.AIS.items() if c.kind == "overflow"}
    assert any(np.isfinite(h).all() and (np.abs(h) > FP32_MAX).any() for h in got.values())
    assert any((~np.isfinite(h)).any() for h in got.values())


def test_ais_a_base_below_fp32s_ulp_is_not_resolved_by_an_fp32_state():
    """The reason diverging-vae-encoder runs with z0_fp32: the statement started from the exact z_0 is more than a gate away, in log w,
    from the one started from z_0 rounded to fp32, on most chains (and more than 10 gates on some), with the same accept sequence."""
    c = SC.AIS["diverging-vae-encoder"]
    assert c.z0_fp32
    _, mu, sg = SC.ais_base(c)
    eps, u = SC.ais_restated_noise(c)
    exact, held = SC.ais_run(dataclasses.replace(c, z0_fp32=False), eps, u), SC.ais_cpu("diverging-vae-encoder")
    d = np.abs(exact["logw"] - held["logw"]).reshape(-1) / np.maximum(1.0, np.abs(held["logw"]).reshape(-1)) / GATE
    print(f"smallest sigma / ulp(mu) of the base {(sg / np.spacing(np.abs(mu))).min():.3f}; |d log w| / gate {np.round(d, 1)}; "
          f"ill-conditioned from the exact start {int((~exact['well']).sum())} of {d.size}")
    assert (sg < np.spacing(np.abs(mu))).any() and np.array_equal(exact["accepts"], held["accepts"])
    assert (d > 1.0).mean() > 0.5 and (d > 10.0).any() and (~exact["well"]).mean() > 0.5 and held["well"].all()


def test_ais_log_w_reaches_1e3_and_1e18():
    big = {n: float(np.abs(SC.ais_cpu(n)["logw"]).max()) for n in SC.AIS}
    print(big)
    assert any(1e3 < v < 1e4 for v in big.values()) and max(big.values()) > 1e18


def test_the_mixture_priors_have_one_dominant_component():
    for table in (SC.AIS, SC.REFINE):
        for n, c in table.items():
            if c.mname == "vae_gmp":
                i = SC.params(c)
                lnpi, _, sg = A.prior_table(i["model"], i["d"], i["p"])
                print(f"{n}: smallest pi {np.exp(lnpi.min()):.3e}, sigma in [{sg.min():.2e}, {sg.max():.2e}]")
                assert lnpi.min() < np.log(1e-30) and lnpi.max() > np.log(0.99)


def test_the_tables_cover_the_shapes():
    for table, sizes in ((SC.AIS, {(4, 16), (3, 5)}), (SC.REFINE, {(5, 4), (19, 1)})):
        small = [c for c in table.values() if c.D < 100 and c.kind == "parity"]
        for regime in SC.REGIMES:
            cs = [c for c in small if c.regime == regime]
            assert {c.D for c in cs} == {23, 24} and {c.L for c in cs} == {3, 5} and {c.act for c in cs} == {"relu", "tanh"}
            assert {c.hidden for c in cs} == {(16,), (12, 20)} and {c.mname for c in cs} == {"vae", "vae_gmp", "gmvae"}
            assert {c.K for c in cs if c.mname != "vae"} == {3, 4}
            assert {(c.B, c.C if table is SC.AIS else c.S) for c in cs} == sizes
            if table is SC.AIS:
                assert {c.init for c in cs} == {"prior", "encoder"}
        big = [c for c in table.values() if c.D == 784]
        assert len(big) == 1 and (big[0].L, big[0].K, big[0].hidden, big[0].regime) == (64, 10, (64,), "trained")


# ================================================================================================================ refinement
@pytest.mark.parametrize("name", list(SC.REFINE))
def test_refine_case(name):
    c, r = SC.REFINE[name], SC.refine_cpu(name)
    kept = r["kept"]
    cnt = r["stats"][:, 5].astype(int)
    g = np.abs(r["grads"])
    gf = np.where(np.isfinite(g), g, 0.0)
    print(f"{name} (rule {SC.refine_rule(c)}): left out {int((~kept).sum())} of {c.B} (undecided {int((~r['decided']).sum())}, "
          f"ill-conditioned {int((~r['well']).sum())}), counts {sorted(set(cnt.tolist()))}, updates clamped at -20 / 5: "
          f"{r['clamped'].sum(axis=0).tolist()}, max |g| {gf.max():.3e}, elbo {r['stats'][:, 0].mean():.4e} -> {r['stats'][:, 1].mean():.4e}")
    assert (~kept).sum() <= SC.CAP * c.B          # (every case: none needed the fall-back that claims no parity)
    assert np.isfinite(r["phi"]).all() and np.isfinite(r["stats"]).all() and np.isfinite(r["tail"]).all()
    skipped = np.zeros((c.n_steps, c.B), bool)
    for t, b in c.inject:
        skipped[t, b] = True
    assert np.array_equal(~np.isfinite(r["trace"]), skipped)           # not finite exactly where the case says so
    s = np.log(r["phi"][:, c.L:])
    assert np.all((s >= RF.S_MIN - 1e-12) & (s <= RF.S_MAX + 1e-12))
    if c.regime == "trained" and c.kind in ("parity", "clamp"):
        assert np.all(cnt == c.n_steps)
    if c.kind == "own_count":
        assert cnt.tolist() == [8, 6, 8, 7, 8] and len(set(cnt[cnt < c.n_steps].tolist())) >= 2
    if c.kind == "clamp":
        lo, hi = SC.clamp_dims(c)
        st = SC.refine_start(c)
        assert np.all(np.log(st[:, c.L + lo].astype(np.float64)) < RF.S_MIN) and np.all(np.log(st[:, c.L + hi].astype(np.float64)) > RF.S_MAX)
        assert r["clamped"][:, 1].all() and (c.regime == "trained" or r["clamped"][:, 0].any())
    if c.kind == "seam":
        b, l = SC.SEAM_EXAMPLE, SC.SEAM_DIM
        in_band = (g > SC.SEAM_BAND[0]) & (g < SC.SEAM_BAND[1])
        want = np.zeros_like(in_band)
        want[:, b, l] = True
        assert np.array_equal(in_band, want) and np.all(g[~want] < float(RF.G_MAX) / 4)      # that one element, nothing near
        assert float(np.float32(g[0, b, l])) ** 2 > FP32_MAX and np.isfinite(np.float32(g[0, b, l]))
        assert cnt[b] == 0 and np.all(np.delete(cnt, b) == c.n_steps)


def test_refine_the_clamp_is_reached_at_each_edge():
    lo = sum(int(SC.refine_cpu(n)["clamped"][:, 0].sum()) for n, c in SC.REFINE.items() if c.kind == "clamp")
    hi = sum(int(SC.refine_cpu(n)["clamped"][:, 1].sum()) for n, c in SC.REFINE.items() if c.kind == "clamp")
    print(f"updates clamped at -20: {lo}, at 5: {hi}")
    assert lo > 0 and hi > 0


def test_refine_the_own_count_case_can_see_a_global_step_index():
    """alpha_t from the step index t + 1 in place of the example's own count: phi* of the two examples that skipped moves by more
    than 10 gates; the examples that skipped nothing do not move at all."""
    c = SC.REFINE["own-count"]
    own = SC.refine_cpu("own-count")
    eps = SC.refine_injected(c, SC.refine_restated_noise(c))
    other = SC.refine_run(c, eps, count="global")
    d = (np.abs(other["phi"] - own["phi"]) / np.maximum(1.0, np.abs(own["phi"]))).max(axis=1) / GATE
    print(f"|d phi*| / gate per example: {d}")
    hit = sorted({b for _, b in c.inject})
    assert np.all(d[hit] > 10.0) and np.all(np.delete(d, hit) == 0.0)


def test_refine_diverging_cases_reach_the_skip_bound_on_their_own():
    """Some example of a diverging case meets a finite gradient of 2^63.5 or more at some step and skips it: the applied counts
    differ within one panel without any injected value."""
    seen = False
    for n, c in SC.REFINE.items():
        if c.regime == "diverging" and c.kind == "parity":
            r = SC.refine_cpu(n)
            cnt = r["stats"][:, 5]
            g = np.abs(r["grads"])
            if len(set(cnt.tolist())) > 1:
                assert np.isfinite(g).all() and (g >= float(RF.G_MAX)).any()
                seen = True
    assert seen
