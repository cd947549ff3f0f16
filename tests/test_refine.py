"""gmvae_refine (include/gmvae_hip.h; csrc/refine.hpp) on the device against the fp64 statement (tests/refine_ref.py): parity of
phi*, the trace and the four bounds on the device's own noise over the three models, the activations, the sample counts, ragged
panels and the size gates' corners; bit-equalities (two calls, in-kernel Philox against supplied noise, the launch split, the batch
split); the skipped update of a gradient that is not finite; n_steps = 0 against Engine.ais_bound; the model surface and the
runner; the memory contract.

Parity holds the DECIDED examples of the statement (refine_ref.refine: every ReLU pre-activation, Adam ratio and clamp clear of its
edge by the margins given there) to 1e-4 max(1, |.|) -- the project's ELBO gate -- and to the count of applied updates exactly, and
a case may leave at most 10 % of its examples undecided.  The shares of the seeds are in profiles/refine_notes.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O
import refine_ref as R
from hip_util import dev, dims_of

pytestmark = pytest.mark.gpu

TOL = 1e-4
P = R.PARITY
KEYS = ("phi", "trace", "stats", "tail")


def _L():
    from gmvae_amd import _lib
    return _lib


def device_noise(n_total, n, Lz, row_base, seed, step):
    """The draws gmvae_refine makes itself, as an array eps [n_total, n, L] (gmvae_noise_fill at step (n_total + 1) + t)."""
    L = _L()
    es = []
    for t in range(n_total):
        e = torch.empty(n, Lz, dtype=torch.float32, device="cuda")
        u = torch.empty(n, 1, dtype=torch.float32, device="cuda")
        L.check(L.lib.gmvae_noise_fill(L.ptr(e), L.ptr(u), n, Lz, 1, row_base, seed, step * (n_total + 1) + t, None,
                                       L.current_stream()), "gmvae_noise_fill")
        es.append(e)
    return torch.stack(es).contiguous()


def device_refine(model, d, flat, x, start, n_steps, S, Rn, eps=None, row0=0, lr=P["lr"], betas=P["betas"], aeps=P["adam_eps"],
                  seed=P["seed"], step=P["step"]):
    """One gmvae_refine call on fresh buffers (the workspace NaN-filled: it needs no initialisation): dict of numpy outputs."""
    L = _L()
    B = x.shape[0]
    cd = dims_of(d, B)
    cd.row0 = row0
    nbytes = L.refine_workspace_bytes(cd, model, S)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(phi=torch.empty(B, 2 * d.L, **f32), trace=torch.empty(max(n_steps, 1), B, **f32), stats=torch.empty(B, 8, **f32),
             tail=torch.empty(L.TAIL, **f32))
    keep = (dev(flat), dev(x), dev(np.asarray(start, np.float32)))
    rc = L.lib.gmvae_refine(C.byref(cd), model, L.ptr(keep[1]), L.ptr(keep[0]), L.ptr(keep[2]), n_steps, S, Rn, lr, betas[0], betas[1],
                            aeps, L.ptr(eps), L.ptr(o["phi"]), L.ptr(o["trace"]), L.ptr(o["stats"]), L.ptr(o["tail"]), L.ptr(ws), seed,
                            step, L.current_stream())
    L.check(rc, "gmvae_refine")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["trace"] = out["trace"][:n_steps]
    return out


def close(got, ref):
    return np.abs(got - ref) <= TOL * np.maximum(1.0, np.abs(ref))


# ----------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", R.CASES, ids=R.cid)
def test_parity_against_the_statement(case):
    model, d, p, flat, x, start, S, n_steps = R.case_inputs(case)
    B = x.shape[0]
    eps = device_noise(n_steps + P["R"], B * S, d.L, 0, P["seed"], P["step"])
    got = device_refine(model, d, flat, x, start, n_steps, S, P["R"], eps)
    ref = R.run_case(case, eps.cpu().numpy())
    dec = ref["decided"]
    err = lambda k, sl=slice(None): np.abs(got[k][..., sl] - ref[k][..., sl])[dec if k != "trace" else slice(None)].max(initial=0)
    print(f"{R.cid(case)}: undecided {int((~dec).sum())} of {B}, max |d phi| {err('phi'):.2e}, |d bounds| {err('stats', slice(0, 4)):.2e}, "
          f"elbo {ref['stats'][:, 0].mean():.3f} -> {ref['stats'][:, 1].mean():.3f}")
    assert (~dec).sum() <= 0.10 * B
    assert np.array_equal(got["stats"][dec, 5], ref["stats"][dec, 5]) and np.all(ref["stats"][:, 5] == n_steps)
    assert np.all(close(got["phi"][dec], ref["phi"][dec]))
    assert np.all(close(got["trace"][:, dec], ref["trace"][:, dec]))
    assert np.all(close(got["stats"][dec, :4], ref["stats"][dec, :4]))
    # the ESS (sum w)^2 / sum w^2: d ln ESS = 2 sum_i (p_i - p2_i) d_i with p, p2 the normalised w and w^2, so log w held to
    # d = TOL max(1, |log w|) holds ln ESS to 4 d
    d_lw = TOL * max(1.0, np.abs(ref["logw_refined"][dec]).max(initial=0))
    assert np.all(np.abs(np.log(got["stats"][dec, 4] / ref["stats"][dec, 4])) <= 4 * d_lw)
    assert np.all(close(got["stats"][dec, 6:], ref["stats"][dec, 6:]))
    if dec.all():
        np.testing.assert_allclose(got["tail"][:5], ref["tail"][:5], rtol=TOL)


# --------------------------------------------------------------------------------------------------------- 2. bit-equalities
def _bits_case():
    d = O.Dims(D=23, L=5, K=3, hidden=(12, 20), act="relu")
    model = O.MODEL_GMVAE
    p, flat, x = R.make(model, d, 4, 77)
    return model, d, flat, x, R.start_table(model, d, p, x).astype(np.float32)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("S", [2, 8])
def test_bit_equalities(S, monkeypatch):
    monkeypatch.delenv("GMVAE_REFINE_LAUNCH_STEPS", raising=False)
    model, d, flat, x, start = _bits_case()      # S = 2: one ragged panel of four examples; S = 8: two panels, one example per half
    n_steps, Rn = 8, 3
    one = device_refine(model, d, flat, x, start, n_steps, S, Rn)
    assert np.all(one["stats"][:, 5] == n_steps) and np.isfinite(one["stats"]).all()
    # two identical calls
    _same(one, device_refine(model, d, flat, x, start, n_steps, S, Rn))
    # in-kernel Philox against the same draws supplied as an array
    eps = device_noise(n_steps + Rn, 4 * S, d.L, 0, P["seed"], P["step"])
    _same(one, device_refine(model, d, flat, x, start, n_steps, S, Rn, eps))
    # 8 steps and 3 rounds in one launch against launches of 3 + 3 + 3 + 2
    monkeypatch.setenv("GMVAE_REFINE_LAUNCH_STEPS", "3")
    _same(one, device_refine(model, d, flat, x, start, n_steps, S, Rn))
    monkeypatch.delenv("GMVAE_REFINE_LAUNCH_STEPS")
    # B = 4 in one call against two calls of B = 2, the second at row0 = 2
    halves = [device_refine(model, d, flat, x[h:h + 2], start[h:h + 2], n_steps, S, Rn, row0=h) for h in (0, 2)]
    for k in ("phi", "stats"):
        assert np.array_equal(np.concatenate([h[k] for h in halves]).view(np.uint8), one[k].view(np.uint8)), k
    assert np.array_equal(np.concatenate([h["trace"] for h in halves], axis=1).view(np.uint8), one["trace"].view(np.uint8))


# ------------------------------------------------------------------------------------------- 3. a gradient that is not finite
def test_a_gradient_that_is_not_finite_skips_that_example_only():
    """Example 1 starts at sigma_0 = inf: z, and so its gradient, is not finite at every step; none of its updates is applied, its
    m stays mu_0, and the other examples' outputs keep their bits."""
    model, d, flat, x, start = _bits_case()
    n_steps, S, Rn = 8, 4, 2
    want = device_refine(model, d, flat, x, start, n_steps, S, Rn)
    bad = start.copy()
    bad[1, d.L:] = np.inf
    got = device_refine(model, d, flat, x, bad, n_steps, S, Rn)
    others = [0, 2, 3]
    for k in ("phi", "stats"):
        assert np.array_equal(got[k][others].view(np.uint8), want[k][others].view(np.uint8)), k
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
    assert np.array_equal(bits(got["trace"][:, others]), bits(want["trace"][:, others]))
    assert got["stats"][1, 5] == 0 and np.all(want["stats"][:, 5] == n_steps)
    assert np.array_equal(got["phi"][1, :d.L], start[1, :d.L]) and np.all(np.isinf(got["phi"][1, d.L:]))
    assert not np.isfinite(got["trace"][:, 1]).any()


# -------------------------------------------------------------------------------------------------------- 4. existing code
@pytest.mark.parametrize("name", ["vae", "vae_gmp"])
def test_no_steps_is_the_encoder_elbo_of_ais_bound(name):
    """n_steps = 0: elbo_start is the mean of Engine.ais_bound(n_temps=1, init="encoder")'s log w on the same supplied eps, and
    iw_start its bound."""
    from gmvae_amd.engine import Engine
    S, Rn, B, Lz = 4, 3, 5, 5
    N = S * Rn
    e = Engine(name, 23, Lz, 1 if name == "vae" else 4, [12, 20], random_seed=3)
    rng = np.random.default_rng(9)
    with torch.no_grad():
        e.params.mul_(2.0)
    x = torch.from_numpy((rng.random((B, 23)) < 0.5).astype(np.uint8)).cuda()
    eps = rng.standard_normal((Rn, B * S, Lz)).astype(np.float32)
    r = e.refine_posterior(x, n_steps=0, n_samples=S, n_eval=N, eps=torch.from_numpy(eps))
    e0 = eps.reshape(Rn, B, S, Lz).transpose(1, 0, 2, 3).reshape(B * N, Lz)          # chain (b, c = r S + s)
    ae = np.stack([e0, rng.standard_normal(e0.shape).astype(np.float32)])
    a = e.ais_bound(x, n_chains=N, n_temps=1, init="encoder", n_leapfrog=2, step_size=0.3, eps=torch.from_numpy(ae),
                    u=torch.from_numpy(rng.random((2, B * N)).astype(np.float32)))
    want = a["logw"].double().mean(dim=1)
    assert torch.all((r["elbo_start"].double() - want).abs() <= TOL * want.abs().clamp_min(1.0))
    assert torch.all((r["iw_start"].double() - a["bound"].double()).abs() <= TOL * a["bound"].double().abs().clamp_min(1.0))
    assert torch.equal(r["elbo_start"], r["elbo_refined"]) and torch.equal(r["iw_start"], r["iw_refined"])
    assert torch.equal(r["phi"][:, :Lz], r["start"][:, :Lz]) and r["trace"].shape == (0, B) and bool((r["updates"] == 0).all())


# ------------------------------------------------------------------------------------------------------ 5. the model surface
def test_model_surface_on_three_models():
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(2)
    x = torch.from_numpy((rng.random((6, 24)) < 0.5).astype(np.uint8)).cuda()
    kw = dict(n_steps=20, n_samples=4, n_eval=32)
    for K in (1, 3):
        m = create_vae(24, 3, mixture_components=K, fcnet_hidden_sizes=[16], random_seed=1)
        g = m.inference_gaps(x, **kw)
        r = m._engine.refine_posterior(x, **kw)
        assert g["elbo_amortised"] == pytest.approx(r["elbo_start"].double().mean().item(), abs=1e-9)
        assert g["elbo_refined"] == pytest.approx(r["elbo_refined"].double().mean().item(), abs=1e-9)
        assert g["log_px"] == pytest.approx(r["iw_refined"].double().mean().item(), abs=1e-9) and g["ais_log_px"] is None
        assert g["amortisation_gap"] == pytest.approx(g["elbo_refined"] - g["elbo_amortised"], abs=1e-9)
        assert g["approximation_gap"] == pytest.approx(g["log_px"] - g["elbo_refined"], abs=1e-9)
        assert g["approximation_gap"] >= -1e-6          # (the importance-weighted bound of the same weights is above their mean)
    m = create_gmvae(24, 3, mixture_components=4, fcnet_hidden_sizes=[16], random_seed=1)
    e = m._engine
    g = m.inference_gaps(x, ais=dict(n_chains=4, n_temps=16, n_leapfrog=3), **kw)
    # the GMVAE's amortised ELBO is the z-marginal one of the inference MIXTURE: the T = 1 path of ais_bound on refine's eval draws
    R_ = kw["n_eval"] // kw["n_samples"]
    t1 = e.ais_bound(x, n_chains=kw["n_eval"], n_temps=1, init="encoder", n_leapfrog=1)
    assert g["elbo_amortised"] == pytest.approx(t1["logw"].double().mean().item(), abs=1e-9) and R_ == 8
    r = e.refine_posterior(x, **kw)
    assert g["elbo_start"] == pytest.approx(r["elbo_start"].double().mean().item(), abs=1e-9)
    a = e.ais_bound(x, n_chains=4, n_temps=16, n_leapfrog=3)["bound"].double().mean().item()
    assert g["ais_log_px"] == pytest.approx(a, abs=1e-9)
    assert g["log_px"] == pytest.approx(max(a, r["iw_refined"].double().mean().item()), abs=1e-9)
    assert g["amortisation_gap"] == pytest.approx(g["elbo_refined"] - g["elbo_amortised"], abs=1e-9)
    assert g["approximation_gap"] == pytest.approx(g["log_px"] - g["elbo_refined"], abs=1e-9)
    assert r["phi"].shape == (6, 6) and r["trace"].shape == (20, 6) and r["stats"].shape == (6, 8) and float(r["tail"][4]) == 6
    assert torch.equal(r["elbo_refined"], r["stats"][:, 1]) and bool((r["updates"] == 20).all())
    for bad in (dict(n_samples=3), dict(n_steps=-1), dict(n_eval=0), dict(lr=0.0), dict(lr=float("nan"))):
        with pytest.raises(ValueError):
            e.refine_posterior(x, **bad)
    with pytest.raises(ValueError):
        e.refine_posterior(x, start=torch.ones(6, 5))
    from gmvae_amd.engine import Engine
    for opt in (dict(pixel_mask=True), dict(likelihood="grey_bernoulli")):
        with pytest.raises(ValueError, match="refine_posterior scores the Bernoulli likelihood"):
            Engine("vae", 24, 3, 1, [16], random_seed=1, **opt).refine_posterior(x)


def test_run_eval_reports_the_inference_gaps(tmp_path):
    """run_gmvae --mode=eval --refine_steps N: the five figures over the whole split, the gap identities, independent of
    --batch_size; with --ais_chains the AIS estimate joins log_px."""
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=128", "--max_steps=20", "--summarise_every=20", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=256"]
    run_gmvae.main(["--mode=train"] + args)
    ref = ["--refine_steps=20", "--refine_samples=2", "--refine_eval_samples=16"]
    res = run_gmvae.main(["--mode=eval"] + args + ref)
    t = lambda k: res[f"train/{k}"]
    assert res["examples"] == 256 and res["refine_stats"].shape == (256, 8)
    assert t("elbo_refined") == pytest.approx(res["refine_stats"][:, 1].double().mean().item(), rel=1e-9)
    assert t("iw_bound_refined") == pytest.approx(res["refine_stats"][:, 3].double().mean().item(), rel=1e-9)
    assert t("amortisation_gap") == pytest.approx(t("elbo_refined") - t("elbo_amortised"), abs=1e-6)
    assert t("approximation_gap") == pytest.approx(t("iw_bound_refined") - t("elbo_refined"), abs=1e-6)
    assert t("approximation_gap") >= 0.0 and -600.0 < t("elbo_amortised") < -100.0
    other = run_gmvae.main(["--mode=eval"] + [a if not a.startswith("--batch_size") else "--batch_size=64" for a in args] + ref)
    assert torch.equal(other["refine_stats"], res["refine_stats"])
    for k in ("elbo_amortised", "elbo_refined", "iw_bound_refined", "amortisation_gap", "approximation_gap"):
        assert other[f"train/{k}"] == t(k), k
    both = run_gmvae.main(["--mode=eval"] + args + ref + ["--ais_chains=2", "--ais_temps=8", "--ais_leapfrog=2"])
    log_px = max(both["train/ais_log_px"], both["train/iw_bound_refined"])
    assert both["train/approximation_gap"] == pytest.approx(log_px - both["train/elbo_refined"], abs=1e-6)
    assert torch.equal(both["refine_stats"], res["refine_stats"])


# ----------------------------------------------------------------------------------------------------- 6. the memory contract
def test_memory_contract_on_guarded_buffers():
    """gmvae_refine on arena buffers at their exact sizes (23 pixels, L = 5, 3 x 4 rows: a ragged panel of several examples; the
    workspace at exactly the bytes its size query answers, 0xFF-filled): nothing changes but the outputs and the workspace, with
    every optional output present and with all of them NULL, and the results are those of the plain call."""
    from arena import Arena
    L = _L()
    model, d, flat, x, start = _bits_case()
    x, start, S, n_steps, Rn, B = x[:3], start[:3], 4, 8, 2, 3
    want = device_refine(model, d, flat, x, start, n_steps, S, Rn)
    cd = dims_of(d, B)
    ar = Arena("cuda", 4 << 20)
    f32 = torch.float32
    ins = {"params": (flat, f32, 4 * 23), "x": (x, torch.uint8, 23), "start": (start, f32, 4 * 2 * d.L)}
    bufs = {}
    for name, (a, dt, pitch) in ins.items():
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dt)
        bufs[name] = ar.place(name, t.numel() * t.element_size(), pitch, False, dt)
        bufs[name].copy_(t)
    outs = {"phi": (B * 2 * d.L, 4 * 2 * d.L), "trace": (n_steps * B, 4 * B), "stats": (8 * B, 32), "tail": (L.TAIL, 4 * L.TAIL)}
    for name, (count, pitch) in outs.items():
        bufs[name] = ar.place(name, 4 * count, pitch, True, f32)
    ws = ar.place("workspace", L.refine_workspace_bytes(cd, model, S), 4 * d.L, True, torch.uint8)
    for with_outputs in (True, False):
        for name in ("phi", "trace", "stats"):
            ar.set_writable(name, with_outputs)
            bufs[name].fill_(float("nan"))
        ws.fill_(0xFF)
        o = (lambda k: L.ptr(bufs[k])) if with_outputs else (lambda k: None)
        ar.snapshot()
        rc = L.lib.gmvae_refine(C.byref(cd), model, L.ptr(bufs["x"]), L.ptr(bufs["params"]), L.ptr(bufs["start"]), n_steps, S, Rn,
                                P["lr"], *P["betas"], P["adam_eps"], None, o("phi"), o("trace"), o("stats"), L.ptr(bufs["tail"]),
                                L.ptr(ws), P["seed"], P["step"], L.current_stream())
        L.check(rc, "gmvae_refine")
        ar.check()
        assert np.array_equal(bufs["tail"].cpu().numpy().view(np.uint8), want["tail"].view(np.uint8))
        if with_outputs:
            for k in ("phi", "trace", "stats"):
                assert np.array_equal(bufs[k].cpu().numpy().view(np.uint8), want[k].reshape(-1).view(np.uint8)), k
