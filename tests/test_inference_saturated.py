"""-m gpu: gmvae_ais (csrc/ais.hpp) and gmvae_refine (csrc/refine.hpp) OUTSIDE the Xavier regime, against their fp64 statements
(tests/ais_ref.py, tests/refine_ref.py) on the cases of tests/inference_saturated_cases.py: parity in the `trained` and `diverging`
regimes; the step-size clips at both ends and the host's clamp of step0; a proposal that is not finite (injected, and reached by
overflow) rejected without a trace; the refinement's own update count beside skipped steps; the clamp of s on both edges and a start
outside it; a gradient whose square is past fp32.

The gate is the parity tests' own (test_ais.TOL = test_refine.TOL = 1e-4 max(1, |.|), accept bits and applied counts exactly), on
the chains or examples the statement ALONE keeps (inference_saturated_cases: DECIDED, well-conditioned), of which a case may leave
out at most 10 %.  Noise is the device's own draws supplied back as arrays, except where a case injects values.  The shares and
the measured errors are in profiles/inference_saturated_notes.md; tests/test_inference_saturated_cpu.py pins each case's
preconditions without a device."""
import math

import numpy as np
import pytest
import torch

import ais_ref as A
import inference_saturated_cases as SC
from test_ais import TOL, accept_matrix, device_ais
from test_ais import device_noise as ais_device_noise
from test_refine import close, device_refine
from test_refine import device_noise as refine_device_noise

pytestmark = pytest.mark.gpu

F32 = np.float32
bits = lambda a: np.ascontiguousarray(a).view(np.uint8)


# ======================================================================================================================= AIS
def _ais_noise(c):
    return ais_device_noise(c.T, c.B * c.C, c.L, 0, SC.SEED, SC.STEP)


def _ais_device(c, eps, u, step0=None):
    i = SC.params(c)
    betas = A.schedule("sigmoid", c.T).astype(F32)
    return device_ais(i["model"], i["d"], i["flat"], i["x"], betas, c.C, c.leap, c.step0 if step0 is None else step0, SC.ais_base(c),
                      eps, u, seed=SC.SEED, step=SC.STEP, up=c.up, down=c.down)


def _steps_from_bits(c, acc, clip=True):
    """The chains' final step sizes from the device's own accept bits, by ais.hpp's recurrence in fp32 (clip=False: without the
    clip to [kAisStepMin, kAisStepMax], to show that the case can tell the two apart)."""
    lo, hi = (F32(A.STEP_MIN), F32(A.STEP_MAX)) if clip else (F32(0), F32(np.inf))
    s = np.full(acc.shape[1], min(max(F32(c.step0), F32(A.STEP_MIN)), F32(A.STEP_MAX)), F32)
    for t in range(c.T):
        s = np.clip((s * np.where(acc[t], F32(c.up), F32(c.down))).astype(F32), lo, hi)
    return s


def _check_ais(name, c, got, ref):
    """test_ais.test_parity_against_the_statement's assertions on the kept chains, the mean step against the statement's, and
    bound, ESS, rate and step by their definitions from the device's own log w and accept bits."""
    kept = ref["kept"]
    acc = accept_matrix(got["bits"], c.T)
    lw_g, lw_r = got["logw"].reshape(-1), ref["logw"].reshape(-1)
    rel = lambda g, r: (np.abs(g - r) / np.maximum(1.0, np.abs(r)))[kept].max(initial=0) / TOL
    print(f"{name}: left out {int((~kept).sum())} of {kept.size} (undecided {int((~ref['decided']).sum())}, ill-conditioned "
          f"{int((~ref['well']).sum())}), accept rate {ref['accepts'].mean():.3f}, max |log w| {np.abs(lw_r).max():.3e}, errors / gate: "
          f"log w {rel(lw_g, lw_r):.3f}, z {rel(got['z'], ref['z']):.3f}")
    assert (~kept).mean() <= SC.CAP
    for k in ("logw", "bound", "stats", "z", "tail"):
        assert np.isfinite(got[k]).all(), k
    assert np.array_equal(acc[:, kept], ref["accepts"][:, kept])
    assert np.all(np.abs(lw_g - lw_r)[kept] <= TOL * np.maximum(1.0, np.abs(lw_r))[kept])
    assert np.all(np.abs(got["z"] - ref["z"])[kept] <= TOL * np.maximum(1.0, np.abs(ref["z"]))[kept])
    whole = kept.reshape(c.B, c.C).all(axis=1)
    np.testing.assert_allclose(got["stats"][whole, 3], ref["steps"].reshape(c.B, c.C).mean(axis=1)[whole], rtol=2e-5)
    # by definition, from the device's own outputs (test_ais.test_stats_and_tail_against_their_definitions)
    lw = got["logw"].astype(np.float64)
    m = lw.max(axis=1, keepdims=True)
    w = np.exp(lw - m)
    bound = m[:, 0] + np.log(w.sum(axis=1)) - math.log(c.C)
    ess = w.sum(axis=1) ** 2 / (w * w).sum(axis=1)
    rate = acc.reshape(c.T, c.B, c.C).mean(axis=(0, 2))
    step = _steps_from_bits(c, acc).astype(np.float64).reshape(c.B, c.C).mean(axis=1)
    np.testing.assert_allclose(got["bound"], bound, rtol=2e-6, atol=2e-6)      # (log w was rounded to fp32 on the way out)
    # (the ESS is taken from log w BEFORE that rounding: half an ulp of |log w| in each weight's exponent moves ln ESS by up to
    # 4 times that -- test_refine's bound for its ESS --, which is the 2e-5 of test_ais wherever |log w| is below 40)
    d_lw = 2.0 ** -24 * np.abs(lw).max(axis=1)
    assert np.all(np.abs(np.log(got["stats"][:, 1] / ess)) <= np.maximum(2e-5, 4 * d_lw))
    np.testing.assert_allclose(got["stats"][:, [0, 2, 3]], np.stack([bound, rate, step], axis=1), rtol=2e-5, atol=2e-6)
    return acc


PARITY_AIS = [n for n, c in SC.AIS.items() if c.kind == "parity"]


@pytest.mark.parametrize("name", PARITY_AIS)
def test_ais_parity(name):
    c = SC.AIS[name]
    eps, u = _ais_noise(c)
    got = _ais_device(c, eps, u)
    ref = SC.ais_run(c, eps.cpu().numpy(), u.cpu().numpy())
    _check_ais(name, c, got, ref)
    rate = ref["accepts"].mean()
    if c.regime == "trained":
        assert 0.0 < rate < 1.0
    elif c.mname != "vae":
        assert rate == 0.0 and not accept_matrix(got["bits"], c.T).any()


# ------------------------------------------------------------------------------------------------------ the step-size clips
def test_ais_step_clip_low():
    """Every proposal rejected from step0 = 2e-4 with down = 0.5: every chain ends at exactly kAisStepMin."""
    c = SC.AIS["clip-low"]
    eps, u = _ais_noise(c)
    got = _ais_device(c, eps, u)
    acc = _check_ais("clip-low", c, got, SC.ais_run(c, eps.cpu().numpy(), u.cpu().numpy()))
    assert not acc.any()
    assert np.all(got["stats"][:, 3] == F32(1e-4))
    assert np.all(_steps_from_bits(c, acc, clip=False) < F32(1e-6))      # (2e-4 / 2^8: without the clip the test would see it)


def test_ais_step_clip_high():
    """From the encoder at step0 = 0.9 with up = 1.5: a chain that accepts is pinned at kAisStepMax."""
    c = SC.AIS["clip-high"]
    eps, u = _ais_noise(c)
    got = _ais_device(c, eps, u)
    ref = SC.ais_run(c, eps.cpu().numpy(), u.cpu().numpy())
    acc = _check_ais("clip-high", c, got, ref)
    with_clip, without = _steps_from_bits(c, acc), _steps_from_bits(c, acc, clip=False)
    pinned = with_clip == F32(1.0)
    print(f"clip-high: {int(acc.any(axis=0).sum())} chains accept, {int(pinned.sum())} end at 1.0, {int((pinned & ref['kept']).sum())} of them kept")
    assert pinned.any() and np.all(without[pinned] > F32(1.0))
    assert (pinned & ref["kept"]).any() and np.array_equal(pinned[ref["kept"]], (ref["steps"] == 1.0)[ref["kept"]])
    ex = pinned.reshape(c.B, c.C).any(axis=1)                          # (stats[:, 3] was held to with_clip's mean at 2e-5 above)
    mean = lambda s: s.astype(np.float64).reshape(c.B, c.C).mean(axis=1)
    assert np.all(np.abs(mean(without) - mean(with_clip))[ex] > 10 * 2e-5 * mean(with_clip)[ex])


def test_ais_step0_is_clamped_on_the_way_in():
    """step0 = 7 and step0 = 1e-6 through the ABI: the results of step0 = 1.0 and of 1e-4, bit for bit (a first transition at 7
    or at 1e-6 would leave other step sizes, and other z, behind)."""
    c = SC.AIS["trained-gmvae-prior"]
    eps, u = _ais_noise(c)
    for outside, edge in ((7.0, 1.0), (1e-6, 1e-4)):
        a, b = _ais_device(c, eps, u, step0=outside), _ais_device(c, eps, u, step0=edge)
        for k in ("logw", "bound", "stats", "z", "tail", "bits"):
            assert np.array_equal(bits(a[k]), bits(b[k])), (outside, k)
    assert accept_matrix(b["bits"], c.T).any()                         # (at 1e-4 chains accept: z has moved by steps of that size)


# --------------------------------------------------------------------------------------- a proposal that is not finite
def test_ais_momentum_of_inf_is_rejected_and_leaves_nothing_behind():
    """eps = inf at transition 3 of chain 3 (a full panel) and chain 18 (the ragged one): the two reject it -- H_new is NaN -- and
    go on from the point they held, to the statement's log w, z_T and later accept bits; every other chain keeps the clean run's
    bits; nothing that is not finite reaches an output."""
    c = SC.AIS["inf-eps"]
    eps, u = _ais_noise(c)
    clean = _ais_device(c, eps, u)
    bad = torch.from_numpy(SC.ais_injected(c, eps.cpu().numpy())).cuda()
    got = _ais_device(c, bad, u)
    ref = SC.ais_run(c, bad.cpu().numpy(), u.cpu().numpy())
    acc = _check_ais("inf-eps", c, got, ref)
    hit = np.zeros(c.B * c.C, bool)
    for t, chain in c.inject:
        hit[chain] = True
        assert not acc[t - 1, chain] and not np.isfinite(ref["h_new"][t - 1, chain])
        assert acc[t:, chain].any()                                    # (a later proposal of the chain was accepted)
    assert ref["kept"][hit].all()
    for k in ("logw", "z", "bits"):
        rows = lambda a: a.reshape(c.B * c.C, -1)[~hit]
        assert np.array_equal(bits(rows(got[k])), bits(rows(clean[k]))), k
    untouched = ~hit.reshape(c.B, c.C).any(axis=1)
    for k in ("bound", "stats"):
        assert np.array_equal(bits(got[k][untouched]), bits(clean[k][untouched])), k


@pytest.mark.parametrize("name", list(SC.OVERFLOW_TWIN))
def test_ais_overflowing_proposals_are_rejected(name):
    """Ten leapfrog steps of 1.0 against sigma = 2e-9: H_new is past fp32 on every chain (NaN or above 3.4e38 in fp64 as well).
    No proposal is accepted, z_T is z_0 -- the all-reject twin's z_T on the same draws, bit for bit --, log w is the statement's,
    and the step size shrank by down^T."""
    c, twin = SC.AIS[name], SC.AIS[SC.OVERFLOW_TWIN[name]]
    eps, u = _ais_noise(c)
    got = _ais_device(c, eps, u)
    ref = SC.ais_run(c, eps.cpu().numpy(), u.cpu().numpy())
    acc = _check_ais(name, c, got, ref)
    past = ~np.isfinite(ref["h_new"]) | (np.abs(ref["h_new"]) > 3.4e38)
    assert past.mean() > 0.5 and not acc.any() and ref["kept"].all()
    z0 = _ais_device(twin, eps, u)
    assert not accept_matrix(z0["bits"], twin.T).any()
    assert np.array_equal(bits(got["z"]), bits(z0["z"]))
    assert np.all(np.abs(got["z"] - ref["z0"]) <= TOL * np.maximum(1.0, np.abs(ref["z0"])))
    np.testing.assert_allclose(got["stats"][:, 3], c.step0 * c.down ** c.T, rtol=2e-5)


# ================================================================================================================ refinement
def _refine_noise(c):
    return refine_device_noise(c.n_steps + SC.ADAM["R"], c.B * c.S, c.L, 0, SC.SEED, SC.STEP)


def _refine_device(c, eps):
    i = SC.params(c)
    P = SC.ADAM
    return device_refine(i["model"], i["d"], i["flat"], i["x"], SC.refine_start(c), c.n_steps, c.S, P["R"], eps, lr=P["lr"],
                         betas=P["betas"], aeps=P["adam_eps"], seed=SC.SEED, step=SC.STEP)


def _sigma_in_range(sigma):
    """sigma* = expf(s) with s in [-20, 5], up to one ulp of expf."""
    lo, hi = F32(np.exp(-20.0)), F32(np.exp(5.0))
    return (sigma >= np.nextafter(lo, F32(0))) & (sigma <= np.nextafter(hi, F32(np.inf)))


def _check_refine(name, c, got, ref):
    """test_refine.test_parity_against_the_statement's assertions on the kept examples (without `== n_steps`: a case may skip),
    a trace that is not finite exactly where the statement's is not, and s within its clamp."""
    kept = ref["kept"]
    L = c.L
    fin = np.isfinite(ref["trace"])
    err = lambda g, r: (np.abs(g - r) / np.maximum(1.0, np.abs(r)))[kept].max(initial=0) / TOL
    tr_g, tr_r = np.where(fin, got["trace"], 0.0).T, np.where(fin, ref["trace"], 0.0).T
    print(f"{name}: left out {int((~kept).sum())} of {c.B} (undecided {int((~ref['decided']).sum())}, ill-conditioned "
          f"{int((~ref['well']).sum())}), counts {sorted(set(ref['stats'][:, 5].astype(int).tolist()))}, clamped at -20 / 5: "
          f"{ref['clamped'].sum(axis=0).tolist()}, max |g| {np.nanmax(np.where(np.isfinite(ref['grads']), np.abs(ref['grads']), 0)):.2e}, "
          f"elbo {ref['stats'][:, 0].mean():.3e} -> {ref['stats'][:, 1].mean():.3e}, errors / gate: phi {err(got['phi'], ref['phi']):.3f}, "
          f"trace {err(tr_g, tr_r):.3f}, bounds {err(got['stats'][:, :4], ref['stats'][:, :4]):.3f}")
    assert (~kept).sum() <= SC.CAP * c.B
    for k in ("phi", "stats", "tail"):
        assert np.isfinite(got[k]).all(), k
    assert np.array_equal(got["stats"][kept, 5], ref["stats"][kept, 5])
    assert np.all(close(got["phi"][kept], ref["phi"][kept]))
    assert np.array_equal(np.isfinite(got["trace"])[:, kept], fin[:, kept])
    assert np.all(close(tr_g[kept], tr_r[kept]))
    assert np.all(close(got["stats"][kept, :4], ref["stats"][kept, :4]))
    d_lw = TOL * max(1.0, np.abs(ref["logw_refined"][kept]).max(initial=0))          # (test_refine: ln ESS is held to 4 d)
    assert np.all(np.abs(np.log(got["stats"][kept, 4] / ref["stats"][kept, 4])) <= 4 * d_lw)
    assert np.all(close(got["stats"][kept, 6:], ref["stats"][kept, 6:]))
    assert np.all(_sigma_in_range(got["phi"][got["stats"][:, 5] > 0, L:]))          # (an example that never updates keeps s_0)
    if kept.all():
        np.testing.assert_allclose(got["tail"][:5], ref["tail"][:5], rtol=TOL)


PARITY_REFINE = [n for n, c in SC.REFINE.items() if c.kind == "parity"]


@pytest.mark.parametrize("name", PARITY_REFINE)
def test_refine_parity(name):
    c = SC.REFINE[name]
    eps = _refine_noise(c)
    got = _refine_device(c, eps)
    ref = SC.refine_run(c, eps.cpu().numpy())
    _check_refine(name, c, got, ref)
    if c.regime == "trained":
        assert np.all(ref["stats"][:, 5] == c.n_steps)


def test_refine_counts_its_own_updates():
    """Example 1 skips steps 2 and 5, example 3 step 0 (eps = inf on their rows): 6, 7 and 8 updates, alpha_t from each example's
    own count -- from the step index the statement is 10 gates and more away (tests/test_inference_saturated_cpu.py) --, the trace
    not finite exactly at the skipped steps, and the examples beside them in the panel keep the clean run's bits."""
    c = SC.REFINE["own-count"]
    eps = _refine_noise(c)
    clean = _refine_device(c, eps)
    bad = torch.from_numpy(SC.refine_injected(c, eps.cpu().numpy())).cuda()
    got = _refine_device(c, bad)
    ref = SC.refine_run(c, bad.cpu().numpy())
    _check_refine("own-count", c, got, ref)
    assert ref["kept"].all()
    assert got["stats"][:, 5].tolist() == [8, 6, 8, 7, 8]
    skipped = np.zeros((c.n_steps, c.B), bool)
    for t, b in c.inject:
        skipped[t, b] = True
    assert np.array_equal(~np.isfinite(got["trace"]), skipped)
    others = [0, 2, 4]
    for k in ("phi", "stats"):
        assert np.array_equal(bits(got[k][others]), bits(clean[k][others])), k
    assert np.array_equal(bits(got["trace"][:, others]), bits(clean["trace"][:, others]))


@pytest.mark.parametrize("name", ["clamp-trained", "clamp-diverging"])
def test_refine_clamp(name):
    """sigma_0 = 2e-9 (s_0 = -20.03) and 200 (s_0 = 5.30) at lr = 0.05: the first update clips, later ones sit on the edge or leave
    it; phi*, the trace and the bounds are the statement's -- elbo_start and iw_start taken at the UNCLAMPED s_0 --, and every
    s* lies in [-20, 5]."""
    c = SC.REFINE[name]
    eps = _refine_noise(c)
    got = _refine_device(c, eps)
    ref = SC.refine_run(c, eps.cpu().numpy())
    _check_refine(name, c, got, ref)
    lo, hi = SC.clamp_dims(c)
    s = np.log(got["phi"][:, c.L:].astype(np.float64))
    print(f"{name}: s* of the two dimensions {s[:, lo]} {s[:, hi]}")
    assert ref["clamped"][:, 1].all() and (ref["clamped"][:, 0].any() or c.regime == "trained")
    # an s* that the statement leaves ON an edge is on it on the device too, to the rounding of sigma* = expf(s*) and back
    on_lo, on_hi = np.log(ref["phi"][:, c.L + lo]) == -20.0, np.log(ref["phi"][:, c.L + hi]) == 5.0
    assert np.all(np.abs(s[:, lo] + 20.0)[on_lo & ref["kept"]] < 1e-6) and np.all(np.abs(s[:, hi] - 5.0)[on_hi & ref["kept"]] < 1e-6)
    assert (on_lo & ref["kept"]).any() or c.regime == "trained"


def test_refine_gradient_whose_square_is_past_fp32():
    """One element's |d m| is 5e19: finite in fp32, its square is not.  The example skips every update (count 0, m* = mu_0) like
    the statement; the examples beside it apply all of theirs."""
    c = SC.REFINE["seam"]
    eps = _refine_noise(c)
    got = _refine_device(c, eps)
    ref = SC.refine_run(c, eps.cpu().numpy())
    _check_refine("seam", c, got, ref)
    want = np.full(c.B, c.n_steps)
    want[SC.SEAM_EXAMPLE] = 0
    assert ref["kept"].all() and np.array_equal(got["stats"][:, 5], want)
    g = np.abs(ref["grads"][:, SC.SEAM_EXAMPLE, SC.SEAM_DIM])
    assert np.all((g > SC.SEAM_BAND[0]) & (g < SC.SEAM_BAND[1]))
    assert np.array_equal(got["phi"][SC.SEAM_EXAMPLE, :c.L], SC.refine_start(c)[SC.SEAM_EXAMPLE, :c.L])
