"""The likelihoods on grey-level bytes (GMVAE_LIK_*) without a device: the fp64 statement (tests/lik_ref.py) against 50-digit
arithmetic, its normalisation, its tie to the Bernoulli statement and the regimes of the device cases; base's distributions; the
library's flag values / schedule names / refusals / workspace; the Python argument checks and the CLI."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import lik_ref as LR
import objective_ref as OR
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = [0.0, 1e-6, -1e-3, 0.04, 0.0499, 0.05, 0.051, -0.3, 1.0, -5.0, 20.0, -60.0, 88.0, -120.0, 1e-30, -1e-30, 100.0, -100.0]


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def r256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ the statement
# (the closed forms cancel: at lambda = 1e-30 the mean's two addends agree in their first 30 digits, so the reference is worked
#  out with 100 guard digits and then read at 50)
def _mp_A(mp, lam):
    with mp.workdps(150):
        lam = mp.mpf(lam)
        v = mp.mpf(0) if lam == 0 else mp.log(mp.expm1(lam) / lam)
    return +v


def _mp_mean(mp, lam):
    with mp.workdps(150):
        lam = mp.mpf(lam)
        v = mp.mpf(1) / 2 if lam == 0 else 1 / (1 - mp.exp(-lam)) - 1 / lam
    return +v


def test_cb_A_and_mean_against_50_digits():
    import mpmath as mp
    mp.mp.dps = 50
    lam = torch.tensor(LAMBDAS, dtype=torch.float64)
    A, M = LR.cb_A(lam).tolist(), LR.cb_mean(lam).tolist()
    for l, a, m in zip(LAMBDAS, A, M):
        ea, em = abs(mp.mpf(a) - _mp_A(mp, l)), abs(mp.mpf(m) - _mp_mean(mp, l))
        print(f"lambda {l:g}: A err {float(ea):.2e} A' err {float(em):.2e}")
        assert ea <= 1e-13 and em <= 1e-13, (l, float(ea), float(em))
    # the autograd Function's backward IS the piecewise A' (finite at 0, where a torch.where over the closed form gives NaN)
    lt = lam.clone().requires_grad_(True)
    LR.family("cb")[0](lt).sum().backward()
    assert torch.equal(lt.grad, LR.cb_mean(lam)) and bool(torch.isfinite(lt.grad).all())


@pytest.mark.parametrize("lam", [-20.0, -1.0, 0.0, 1e-3, 5.0, 50.0])
def test_cb_is_normalised(lam):
    import mpmath as mp
    mp.mp.dps = 50
    A = mp.mpf(LR.cb_A(torch.tensor(lam, dtype=torch.float64)).item())
    integral = mp.quad(lambda t: mp.exp(t * mp.mpf(lam) - A), [0, 1])
    assert abs(integral - 1) <= 1e-13, (lam, float(integral - 1))


@pytest.mark.parametrize("mname", ["vae", "vae_gmp", "gmvae"])
@pytest.mark.parametrize("S", [1, 3])
def test_grey_on_0_255_is_the_bernoulli_statement(mname, S):
    """255 / 255 is exactly 1: with grey_bernoulli and x in {0, 255} the statement is objective_ref's on x in {0, 1}."""
    model = O.MODEL_NAMES[mname]
    d = O.Dims(D=40, L=4, K=1 if mname == "vae" else 5, hidden=(12,), S=S, temperature=0.8)
    p = O.init_params(model, d, np.random.default_rng(2))
    x, eps, u = O.make_inputs(d, 6, model)
    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    co, go = OR.loss_and_grads(model, d, p, x, eps, OR.iwae, S=S, **kw)
    Cs, gs = LR.loss_and_grads(model, d, p, (x * 255).astype(np.uint8), eps, u if model == O.MODEL_GMVAE else None, "grey")
    assert abs(Cs["loss"] - co["loss"]) <= 1e-12 * max(abs(co["loss"]), 1.0)
    assert abs(Cs["nll"] + co["logpx"].mean().item()) <= 1e-12 * abs(Cs["nll"])
    for k in go:
        assert np.abs(gs[k] - go[k]).max() <= 1e-12 * max(np.abs(go[k]).max(), 1.0), k


_STMT = {}


def _statement(name):
    if name not in _STMT:
        model, d, p, flat, x, eps, u = LR.setup(name)
        c = LR.CASES[name]
        _STMT[name] = LR.loss_and_grads(model, d, p, x, eps, u, c.lik, c.sigma)
    return _STMT[name]


@pytest.mark.parametrize("name", list(LR.CASES))
def test_case_regimes(name):
    """Every case has a finite statement and sits in the regime its name says."""
    model, d, p, flat, x, eps, u = LR.setup(name)
    c = LR.CASES[name]
    Cc, g = _statement(name)
    assert x.dtype == np.uint8 and x.shape == (c.B, d.D) and (x == 0).mean() > 0.2 and (x == 255).mean() > 0.05 and len(np.unique(x)) > 100
    assert all(np.isfinite(Cc[k]) for k in ("loss", "nll", "kl", "nent", "sqerr", "nll_abs")) and np.isfinite(Cc["rows"]).all()
    assert all(np.isfinite(v).all() for v in g.values())
    assert Cc["nll_abs"] >= abs(Cc["nll"]) * (1 - 1e-12) and Cc["sqerr"] >= 0
    top = np.abs(Cc["lam"]).max()
    print(f"{name}: max |lambda| {top:.4g} loss {Cc['loss']:.6g} nll {Cc['nll']:.6g} nll_abs {Cc['nll_abs']:.6g} sqerr {Cc['sqerr']:.6g}")
    if name == "vae-cb-tiny":
        assert 0 < top <= 1e-3
    if name == "vae-cb-saturated":
        assert 50.0 <= top <= 70.0
    if name == "vae-cb-100":
        assert 90.0 <= top <= 110.0
    if name == "vae-cb-zero":
        t = LR.targets(x)
        nl = len(d.hidden)
        assert top == 0.0 and (Cc["rows"][:, 0] == 0).all()
        assert np.abs(g[f"decoder_fcnet/linear_{nl}/b"].reshape(-1) - (0.5 - t).sum(axis=0) / c.B).max() <= 1e-14
        assert abs(Cc["sqerr"] - ((0.5 - t) ** 2).sum()) <= 1e-12 * Cc["sqerr"]
    if c.lik == "cb":
        assert (Cc["mean"] > 0).all() and (Cc["mean"] < 1).all()


def test_gaussian_statement_is_the_normal_log_density():
    model, d, p, flat, x, eps, u = LR.setup("vae-gauss-sigma-small")
    Cc, _ = _statement("vae-gauss-sigma-small")
    s, t = LR.CASES["vae-gauss-sigma-small"].sigma, LR.targets(x)
    ref = (-0.5 * ((t - Cc["lam"]) / s) ** 2 - np.log(s) - 0.5 * np.log(2 * np.pi)).sum(axis=1)
    assert np.abs(Cc["rows"][:, 0] - ref).max() <= 1e-11 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ base's distributions
def test_base_distributions_against_the_statement():
    from gmvae_amd import base
    lam64 = torch.tensor([0.0, 1e-6, -1e-6, 1e-3, -1e-3, 1.0, -1.0, 60.0, -60.0, 100.0, -100.0], dtype=torch.float64)
    t64 = torch.linspace(0.0, 1.0, lam64.numel(), dtype=torch.float64)
    cb = base.ContinuousBernoulli(lam64.float()[None, :])
    ref_lp = (t64 * lam64 - LR.cb_A(lam64)).sum()
    ref_abs = (t64 * lam64 - LR.cb_A(lam64)).abs().sum()
    assert torch.isfinite(cb.mean()).all()
    assert (cb.mean()[0].double() - LR.cb_mean(lam64)).abs().max() <= 1e-6
    assert abs(cb.log_prob(t64.float()[None, :]).item() - ref_lp.item()) <= 1e-6 * ref_abs.item()
    per = (t64.float() * lam64.float() - base._cb_terms(lam64.float())[0]).double()
    assert ((per - (t64 * lam64 - LR.cb_A(lam64))).abs() <= 1e-6 * (t64 * lam64 - LR.cb_A(lam64)).abs().clamp(min=1.0)).all()
    n = base.NormalFixedScale(lam64.float()[None, :], 0.25)
    A, Ap, phi, cfn = LR.family("gauss", 0.25)
    ref = ((t64 * lam64 - A(lam64)) / phi + cfn(t64))
    assert torch.equal(n.mean()[0], lam64.float())
    assert abs(n.log_prob(t64.float()[None, :]).item() - ref.sum().item()) <= 1e-6 * ref.abs().sum().item()
    # Bernoulli.log_prob accepts soft targets
    b = base.Bernoulli(lam64.float()[None, :])
    refb = (t64 * lam64 - torch.nn.functional.softplus(lam64))
    assert abs(b.log_prob(t64.float()[None, :]).item() - refb.sum().item()) <= 1e-6 * refb.abs().sum().item()


@pytest.mark.parametrize("lam", [-3.0, 0.0, 2.0])
def test_sample_means(lam):
    from gmvae_amd import base
    N = 200000
    lt = torch.full((N,), lam)
    s = base.ContinuousBernoulli(lt).sample(seed=3).double()
    assert bool(((s >= 0) & (s <= 1)).all())
    m = LR.cb_mean(torch.tensor(lam, dtype=torch.float64)).item()
    assert abs(s.mean().item() - m) <= 4 * s.std().item() / N ** 0.5, (s.mean().item(), m)
    g = base.NormalFixedScale(lt, 0.5).sample(seed=4).double()
    assert abs(g.mean().item() - lam) <= 4 * 0.5 / N ** 0.5 and abs(g.std().item() - 0.5) < 0.01


# ------------------------------------------------------------------------------------------------ the library
def test_flag_values_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    for name, val in (("GMVAE_LIK_GREY_BERNOULLI", 1 << 11), ("GMVAE_LIK_CONT_BERNOULLI", 2 << 11), ("GMVAE_LIK_GAUSSIAN", 3 << 11),
                      ("GMVAE_LIK_MASK", 3 << 11)):
        m = re.search(name + r"\s*=\s*(\d+)\s*<<\s*(\d+)", hdr)
        assert m and int(m.group(1)) << int(m.group(2)) == val, name
    assert (L.LIK_GREY_BERNOULLI, L.LIK_CONT_BERNOULLI, L.LIK_GAUSSIAN, L.LIK_MASK) == (2048, 4096, 6144, 6144)
    assert L.LIK_MASK & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG | L.OBJ_LABELS |
                         L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH | L.OBJ_PIXEL_MASK | L.OPT_CLIP_NORM) == 0
    assert {LR.FLAG[k] for k in LR.LIKS} == {L.LIK_GREY_BERNOULLI, L.LIK_CONT_BERNOULLI, L.LIK_GAUSSIAN}
    assert L.LIKELIHOODS == {"bernoulli": 0, **{LR.NAME[k]: LR.FLAG[k] for k in LR.LIKS}}
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


def test_schedule_names(L):
    """With the field every step takes the general schedule: at the one-launch sizes, the skinny sizes, the one-launch VAE sizes
    and the config-5 sizes (no "+planes"); "+clip" composes."""
    for lik in LR.LIKS:
        F, sfx = LR.FLAG[lik], LR.SUFFIX[lik]
        gm = lambda fl, B=1024: L.step_schedule(L.make_dims(B, 784, 64, 10, (64,), sched_flags=fl), L.MODEL_GMVAE)
        assert gm(0) != "general" and gm(F) == "general" + sfx and gm(F, 16) == "general" + sfx
        sk = lambda fl: L.step_schedule(L.make_dims(64, 784, 128, 10, (512,), sched_flags=fl), L.MODEL_GMVAE)
        assert sk(0) == "skinny" and sk(F) == "general" + sfx
        c5 = lambda fl: L.step_schedule(L.make_dims(25600, 3072, 128, 64, (512, 512), sched_flags=fl), L.MODEL_GMVAE)
        assert c5(0) == "general+planes" and c5(F) == "general" + sfx
        va = lambda fl: L.step_schedule(L.make_dims(1024, 784, 2, 1, (64,), sched_flags=fl), L.MODEL_VAE)
        assert va(0) != "general" and va(F) == "general" + sfx
        gp = lambda fl: L.step_schedule(L.make_dims(1024, 784, 64, 10, (64,), sched_flags=fl), L.MODEL_VAE_GMP)
        assert gp(0) != "general" and gp(F) == "general" + sfx
        assert gm(F | L.OPT_CLIP_NORM) == "general" + sfx + "+clip"
        assert L.step_schedule(L.make_dims(8, 96, 4, 6, (16,), S=3, sched_flags=F), L.MODEL_GMVAE) == "general" + sfx


def _offset(L, d, model, name):
    o = C.c_uint64()
    return L.lib.gmvae_workspace_offset(C.byref(d), model, name, C.byref(o)), o.value


WS_DIMS = [   # (model, B, D, Lz, K, hidden, S)
    ("gmvae", 1024, 784, 64, 10, (64,), 1), ("gmvae", 5, 99, 5, 7, (24,), 1), ("gmvae", 4, 96, 4, 6, (16,), 3),
    ("vae", 9, 100, 5, 1, (24,), 1), ("vae_gmp", 9, 100, 5, 3, (24,), 1), ("vae", 3, 1, 2, 1, (4,), 2),
]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"{c[0]}-B{c[1]}-D{c[2]}-S{c[6]}")
def test_workspace_grows_behind_everything(L, case):
    """With the field: + r256(4 B D) (t) + r256(4 R ceil(D / 32)) (the squared-error partials), + 256 (sigma's cell) under the
    Gaussian, behind every other buffer; no other offset moves; "lik_sigma" resolves under the Gaussian alone and lies apart
    from "clip_norm" / "grad_clip", which keep resolving."""
    mname, B, D, Lz, K, hidden, S = case
    model = L.MODEL_IDS[mname]
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=f)
    base = L.workspace_bytes(mk(0), model)
    grow = r256(4 * B * D) + r256(4 * B * S * ((D + 31) // 32))
    for lik in LR.LIKS:
        F = LR.FLAG[lik]
        assert L.workspace_bytes(mk(F), model) - base == grow + (256 if lik == "gauss" else 0), lik
        for buf in (b"z", b"dqp", b"slabs", b"logw", b"logq", b"g", b"eps"):
            a = _offset(L, mk(0), model, buf)
            assert a == _offset(L, mk(F), model, buf) and a[0] == 0 and a[1] < base, buf
        rc, off = _offset(L, mk(F), model, b"lik_sigma")
        if lik != "gauss":
            assert rc == -5
            continue
        # (sigma's cell opens the trailing regions: where "clip_norm" starts in the layout without the field)
        assert rc == 0 and off % 256 == 0 and off == _offset(L, mk(L.OPT_CLIP_NORM), model, b"clip_norm")[1]
        assert off + 256 + grow <= L.workspace_bytes(mk(F), model)
        both = mk(F | L.OPT_CLIP_NORM)
        total = L.workspace_bytes(both, model)
        (r0, s0), (r1, c0), (r2, g0) = (_offset(L, both, model, n) for n in (b"lik_sigma", b"clip_norm", b"grad_clip"))
        assert r0 == r1 == r2 == 0 and s0 == off and s0 + 256 <= c0 and c0 + 256 <= g0 and g0 + 16 * L.LABEL_SLOTS <= total
        assert min(c0, g0) >= s0 + 256 + grow
    assert _offset(L, mk(0), model, b"lik_sigma")[0] == -5


def test_workspace_without_the_field_is_the_recorded_size(L):
    with open(os.path.join(ROOT, "tests", "golden", "step_inputs_layout.json")) as f:
        gold = json.load(f)
    seen = 0
    for c in gold["cases"]:
        assert not c["flags"] & L.LIK_MASK
        d = L.make_dims(c["B"], c["D"], c["L"], c["K"], c["hidden"], S=c["S"], sched_flags=c["flags"])
        assert L.workspace_bytes(d, L.MODEL_IDS[c["model"]]) == c["bytes"], c
        seen += 1
    assert seen >= 3


def test_refusals_by_code(L):
    """GMVAE_E_DIMS together with every other objective / estimator bit, from every entry that sizes or runs a step, before
    anything is touched (every pointer here is a host dummy); the pipeline graph, and the three evaluators that would score
    Bernoulli."""
    u64 = C.c_uint64()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    G = L.MODEL_GMVAE
    h = C.c_void_p()
    for lik in LR.LIKS:
        M = LR.FLAG[lik]
        mk = lambda S, f, K=10: L.make_dims(16, 784, 8, K, (64,), S=S, sched_flags=f)
        oks = [(mk(1, M), G), (mk(3, M), G), (mk(1, M, 1), L.MODEL_VAE), (mk(2, M), L.MODEL_VAE_GMP), (mk(1, M | L.OPT_CLIP_NORM), G)]
        for d, model in oks:
            assert L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
            assert L.lib.gmvae_iw_bound_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
        cases = [(mk(1, M | L.OBJ_MARGINAL_Y), G), (mk(2, M | L.OBJ_MARGINAL_Y_IW), G), (mk(2, M | L.GRAD_DREG, 1), L.MODEL_VAE),
                 (mk(1, M | L.GRAD_DREG | L.OBJ_MARGINAL_Y), G), (mk(1, M | L.OBJ_LABELS | L.OBJ_MARGINAL_Y), G),
                 (mk(1, M | L.OBJ_WEIGHTS), G), (mk(1, M | L.OBJ_WEIGHTS, 1), L.MODEL_VAE), (mk(1, M | L.Y_TEMP_DEV), G),
                 (mk(3, M | L.Y_STRAIGHT_THROUGH), G), (mk(1, M | L.OBJ_PIXEL_MASK), G), (mk(2, M | L.OBJ_PIXEL_MASK, 1), L.MODEL_VAE)]
        for d, model in cases:
            r = C.byref(d)
            assert L.lib.gmvae_workspace_bytes(r, model, C.byref(u64)) == -2
            assert L.lib.gmvae_workspace_offset(r, model, b"lik_sigma", C.byref(u64)) == -2
            assert L.lib.gmvae_step_schedule(r, model, C.create_string_buffer(48)) == -2
            assert L.lib.gmvae_step(r, model, p, None, None, p, p, p, 0, 0, None, None) == -2
            assert L.lib.gmvae_forward(r, model, p, None, None, p, p, None, None, None, None, p, 0, 0, None) == -2
            assert L.lib.gmvae_train_graph_create(r, model, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, C.byref(C.c_void_p())) == -2
            assert L.lib.gmvae_dp_step(r, model, p, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None) == -2
            assert L.lib.gmvae_dp_graph_create(r, model, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None,
                                               C.byref(C.c_void_p())) == -2
            assert L.lib.gmvae_bench_loop(r, model, p, p, p, p, p, p, p, 1, 0, C.byref(C.c_float()), None) == -2
            assert L.lib.gmvae_iw_bound_workspace_bytes(r, model, C.byref(u64)) == -2
            assert L.lib.gmvae_iw_bound(r, model, p, p, 4, None, None, p, p, 0, 0, None) == -2
        for d, model in oks[:4]:
            assert L.lib.gmvae_train_graph_create_pipeline(C.byref(d), model, p, 100, p, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999,
                                                           1e-8, None, C.byref(h)) == -2
        # the evaluators that would score Bernoulli
        d = mk(2, M)
        r = C.byref(d)
        assert L.lib.gmvae_iw_bound_enum_y_workspace_bytes(r, G, C.byref(u64)) == -2
        assert L.lib.gmvae_posterior_y_workspace_bytes(r, G, C.byref(u64)) == -2
        assert L.lib.gmvae_posterior_component_workspace_bytes(r, L.MODEL_VAE_GMP, C.byref(u64)) == -2
        assert L.lib.gmvae_iw_bound_enum_y(r, G, p, p, 4, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_posterior_y(r, G, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_posterior_component(r, L.MODEL_VAE_GMP, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
    assert h.value is None


def test_iw_bound_workspace_holds_the_likelihood_regions(L):
    """gmvae_iw_bound honours the field: its workspace opens with the forward's, sigma's cell at the same offset."""
    mk = lambda f: L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=f)
    F = L.LIK_GAUSSIAN
    a, b = L.iw_bound_workspace_bytes(mk(0), L.MODEL_GMVAE), L.iw_bound_workspace_bytes(mk(F), L.MODEL_GMVAE)
    assert b - a == L.workspace_bytes(mk(F), L.MODEL_GMVAE) - L.workspace_bytes(mk(0), L.MODEL_GMVAE)


# ------------------------------------------------------------------------------------------ the Python surface
def test_check_likelihood(L):
    from gmvae_amd.engine import check_likelihood
    ok = ("gmvae", "gumbel", "standard", False, False, False, "relaxed", False)
    for name in L.LIKELIHOODS:
        assert check_likelihood(*ok, name, 0.25) == 0.25
        assert check_likelihood("vae", *ok[1:], name) == 1.0
    check_likelihood("gmvae", "marginal_iw", "dreg", True, True, True, "straight_through", True, "bernoulli")      # off: nothing to refuse
    with pytest.raises(ValueError, match="likelihood must be one of"):
        check_likelihood(*ok, "poisson")
    for bad in (0.0, -1.0, float("inf"), float("nan"), "wide", None):
        with pytest.raises(ValueError, match="likelihood_sigma"):
            check_likelihood(*ok, "gaussian", bad)
    bad = [(("gmvae", "marginal", "standard", False, False, False, "relaxed", False), "y_inference"),
           (("gmvae", "marginal_iw", "standard", False, False, False, "relaxed", False), "y_inference"),
           (("vae", "gumbel", "dreg", False, False, False, "relaxed", False), "dreg"),
           (("gmvae", "gumbel", "standard", True, False, False, "relaxed", False), "semi_supervised"),
           (("gmvae", "gumbel", "standard", False, True, False, "relaxed", False), "weighted_objective"),
           (("gmvae", "gumbel", "standard", False, False, True, "relaxed", False), "temperature_on_device"),
           (("gmvae", "gumbel", "standard", False, False, False, "straight_through", False), "y_estimator"),
           (("vae", "gumbel", "standard", False, False, False, "relaxed", True), "pixel_mask")]
    for args, what in bad:
        for name in ("grey_bernoulli", "continuous_bernoulli", "gaussian"):
            with pytest.raises(ValueError, match=what):
                check_likelihood(*args, name)


def test_engine_refuses_before_it_needs_a_device(L):
    """Engine's argument checks come first: they raise ValueError with or without a device."""
    from gmvae_amd.engine import Engine
    with pytest.raises(ValueError, match="likelihood_sigma"):
        Engine("vae", 20, 2, 1, [8], likelihood="gaussian", likelihood_sigma=0.0)
    with pytest.raises(ValueError, match="pixel_mask"):
        Engine("vae", 20, 2, 1, [8], likelihood="continuous_bernoulli", pixel_mask=True)
    with pytest.raises(ValueError, match="likelihood must be one of"):
        Engine("vae", 20, 2, 1, [8], likelihood="laplace")
    with pytest.raises(ValueError, match="y_inference"):
        Engine("gmvae", 20, 2, 3, [8], likelihood="grey_bernoulli", y_inference="marginal")


def test_runner_flags(L):
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    d = run_gmvae.check_args(p, p.parse_args([]))
    assert d.likelihood == "bernoulli" and d.likelihood_sigma == 1.0 and not runners.grey_levels(d)
    ok = run_gmvae.check_args(p, p.parse_args(["--likelihood=gaussian", "--likelihood_sigma=0.25", "--iw_samples=7", "--n_samples=3",
                                               "--clip_norm=5"]))
    assert runners.likelihood_of(ok) == ("gaussian", 0.25) and runners.grey_levels(ok)
    run_gmvae.check_args(p, p.parse_args(["--model=vae_gmp", "--likelihood=continuous_bernoulli"]))
    run_gmvae.check_args(p, p.parse_args(["--model=vae", "--likelihood=grey_bernoulli"]))
    lk = "--likelihood=continuous_bernoulli"
    for bad in ([lk, "--y_inference=marginal"], [lk, "--y_inference=marginal_iw"], [lk, "--model=vae", "--grad_estimator=dreg"],
                [lk, "--kl_weight=0.5"], [lk, "--kl_warmup_steps=10"], [lk, "--temperature=0.5"], [lk, "--y_estimator=straight_through"],
                [lk, "--iw_enum_samples=4"], [lk, "--posterior_samples=4"], [lk, "--missing_rate=0.5"],
                [lk, "--model=vae_gmp", "--mode=eval", "--component_posterior_samples=4"],
                ["--likelihood=gaussian", "--likelihood_sigma=0"], ["--likelihood=gaussian", "--likelihood_sigma=-1"],
                ["--likelihood=gaussian", "--likelihood_sigma=inf"], ["--likelihood=poisson"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    g = runners.synthetic_grey(64, 50)
    assert g.dtype == np.uint8 and g.shape == (64, 50) and np.array_equal(g, runners.synthetic_grey(64, 50)) and len(np.unique(g)) > 50
