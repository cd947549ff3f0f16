"""Real-valued data and the learned Gaussian scale (GMVAE_X_F32, GMVAE_LIK_SCALE_LEARNED) without a device: the library's flag
values / schedule names / parameter layout / workspace / refusals, the Python and runner argument checks, and the anchors of
the fp64 statement (tests/realx_ref.py): its tie to lik_ref's Gaussian and the rho gradient against central differences."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import lik_ref as LR
import oracle as O
import realx_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def r256(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ the library
def test_flag_values_header_text_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    for name, val in (("GMVAE_X_F32", 1 << 13), ("GMVAE_LIK_SCALE_LEARNED", 1 << 14)):
        m = re.search(name + r"\s*=\s*(\d+)\s*<<\s*(\d+)", hdr)
        assert m and int(m.group(1)) << int(m.group(2)) == val, name
    assert (L.X_F32, L.LIK_SCALE_LEARNED) == (RR.X_F32, RR.LIK_SCALE_LEARNED) == (8192, 16384)
    assert RR.LIK_GAUSSIAN == L.LIK_GAUSSIAN and L.LOG_SIGMA == RR.LOG_SIGMA == "decoder/log_sigma"
    others = (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG | L.OBJ_LABELS |
              L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH | L.OBJ_PIXEL_MASK | L.OPT_CLIP_NORM | L.LIK_MASK)
    assert (L.X_F32 | L.LIK_SCALE_LEARNED) & others == 0
    # the header documents the reinterpretation of x, the alignment, the new entry and the schedule suffixes
    for text in ("const float*", "16-byte aligned", "GMVAE_E_ALIGN", "decoder/log_sigma", "sigma_d = exp(rho_d)", '"+f32"', '"+lsig"'):
        assert text in hdr, text
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION
    assert L.LIKELIHOODS == {"bernoulli": 0, **{LR.NAME[k]: LR.FLAG[k] for k in LR.LIKS}}      # (untouched)


def test_schedule_names(L):
    G, F, S = L.LIK_GAUSSIAN, L.X_F32, L.LIK_SCALE_LEARNED
    for mk, model in ((lambda fl: L.make_dims(1024, 784, 64, 10, (64,), sched_flags=fl), L.MODEL_GMVAE),
                      (lambda fl: L.make_dims(64, 784, 128, 10, (512,), sched_flags=fl), L.MODEL_GMVAE),
                      (lambda fl: L.make_dims(25600, 3072, 128, 64, (512, 512), sched_flags=fl), L.MODEL_GMVAE),
                      (lambda fl: L.make_dims(1024, 784, 2, 1, (64,), sched_flags=fl), L.MODEL_VAE),
                      (lambda fl: L.make_dims(8, 96, 4, 6, (16,), S=3, sched_flags=fl), L.MODEL_VAE_GMP)):
        assert L.step_schedule(mk(G), model) == "general+gauss"
        assert L.step_schedule(mk(G | F), model) == "general+gauss+f32"
        assert L.step_schedule(mk(G | S), model) == "general+gauss+lsig"
        assert L.step_schedule(mk(G | F | S), model) == "general+gauss+f32+lsig"
        assert L.step_schedule(mk(G | F | S | L.OPT_CLIP_NORM), model) == "general+gauss+f32+lsig+clip"


LAYOUT_DIMS = [("gmvae", 5, 99, 5, 7, (24,)), ("gmvae", 32, 784, 64, 10, (64,)), ("vae", 1, 3, 2, 1, (8,)), ("vae_gmp", 9, 100, 5, 3, (24,))]


@pytest.mark.parametrize("case", LAYOUT_DIMS, ids=lambda c: f"{c[0]}-D{c[2]}")
def test_parameter_layout(L, case):
    """The extra entry comes last, P grows by pad4(D), and without the bit the layout is identical -- under the bit alone."""
    mname, B, D, Lz, K, hidden = case
    model = L.MODEL_IDS[mname]
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, sched_flags=f)
    base_lay, (P0, R0) = L.param_layout(mk(0), model), L.param_count(mk(0), model)
    for f in (L.LIK_GAUSSIAN, L.LIK_GAUSSIAN | L.X_F32, L.X_F32, L.LIK_MASK, L.OPT_CLIP_NORM):
        assert L.param_layout(mk(f), model) == base_lay and L.param_count(mk(f), model) == (P0, R0)
    for f in (L.LIK_SCALE_LEARNED, L.LIK_SCALE_LEARNED | L.LIK_GAUSSIAN, L.LIK_SCALE_LEARNED | L.LIK_GAUSSIAN | L.X_F32):
        lay = L.param_layout(mk(f), model)
        assert lay[:-1] == base_lay and lay[-1] == (L.LOG_SIGMA, (1, D), P0)
        assert L.param_count(mk(f), model) == (P0 + RR.pad4(D), R0 + D)


def _offset(L, d, model, name):
    o = C.c_uint64()
    return L.lib.gmvae_workspace_offset(C.byref(d), model, name, C.byref(o)), o.value


def test_workspace_without_the_bits_is_the_recorded_size(L):
    with open(os.path.join(ROOT, "tests", "golden", "step_inputs_layout.json")) as f:
        gold = json.load(f)
    seen = 0
    for c in gold["cases"]:
        assert not c["flags"] & (L.X_F32 | L.LIK_SCALE_LEARNED)
        d = L.make_dims(c["B"], c["D"], c["L"], c["K"], c["hidden"], S=c["S"], sched_flags=c["flags"])
        assert L.workspace_bytes(d, L.MODEL_IDS[c["model"]]) == c["bytes"], c
        seen += 1
    assert seen >= 3


WS_DIMS = [("gmvae", 1024, 784, 64, 10, (64,), 1), ("gmvae", 5, 99, 5, 7, (24,), 1), ("gmvae", 4, 96, 4, 6, (16,), 3),
           ("vae", 1, 3, 2, 1, (8,), 1), ("vae_gmp", 9, 100, 5, 3, (24,), 2)]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"{c[0]}-B{c[1]}-D{c[2]}-S{c[6]}")
def test_workspace_regions(L, case):
    """GMVAE_X_F32: the t region [B D] is gone; the learned scale: sigma's cell is gone ("lik_sigma" does not resolve), the slab
    partials of the rho reduction come in, and the split-K slabs grow with P.  No other offset in front of the slabs moves."""
    mname, B, D, Lz, K, hidden, S = case
    model = L.MODEL_IDS[mname]
    G, F, SL = L.LIK_GAUSSIAN, L.X_F32, L.LIK_SCALE_LEARNED
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=f)
    wb = lambda f: L.workspace_bytes(mk(f), model)
    assert wb(G) - wb(G | F) == r256(4 * B * D)
    assert wb(G | SL) - wb(G | F | SL) == r256(4 * B * D)
    for buf in (b"z", b"dqp", b"logw", b"logq", b"g", b"eps", b"slabs"):
        a = _offset(L, mk(G), model, buf)
        assert a[0] == 0 and a == _offset(L, mk(G | F), model, buf) == _offset(L, mk(G | SL), model, buf), buf
    assert _offset(L, mk(G), model, b"lik_sigma")[0] == 0 and _offset(L, mk(G | F), model, b"lik_sigma")[0] == 0
    assert _offset(L, mk(G | SL), model, b"lik_sigma")[0] == -5 and _offset(L, mk(G | F | SL), model, b"lik_sigma")[0] == -5
    # the rho reduction's partials: ceil(R / 64) slabs (at most 256) of pad4(D) floats; the slabs: (their count) x pad4(D) more
    R = B * S
    rs = 64
    while (R + rs - 1) // rs > 256:
        rs *= 2
    part = r256(4 * ((R + rs - 1) // rs) * RR.pad4(D))
    grown = wb(G | SL) - wb(G) + 256 - part
    assert grown >= 0 and grown % 256 == 0 and grown >= 4 * RR.pad4(D) - 255
    both = mk(G | F | SL | L.OPT_CLIP_NORM)
    (r1, c0), (r2, g0) = _offset(L, both, model, b"clip_norm"), _offset(L, both, model, b"grad_clip")
    assert r1 == r2 == 0 and c0 + 256 <= g0 and g0 + 16 * L.LABEL_SLOTS <= L.workspace_bytes(both, model)
    # gmvae_iw_bound's workspace opens with the forward's
    a, b = L.iw_bound_workspace_bytes(mk(G), model), L.iw_bound_workspace_bytes(mk(G | F), model)
    assert a - b == r256(4 * B * D)


def test_refusals_by_code(L):
    """GMVAE_E_DIMS from every entry that sizes or runs a step, before anything is touched (every pointer here is a host dummy):
    either bit without the Gaussian, every bit check_lik_dims refuses, the pipeline graph, the three enumerating evaluators;
    GMVAE_E_ALIGN for an x that is not 16-byte aligned under GMVAE_X_F32."""
    u64 = C.c_uint64()
    buf = C.create_string_buffer(4096 + 16)
    base = (C.addressof(buf) + 15) // 16 * 16
    p, p4 = C.c_void_p(base), C.c_void_p(base + 4)
    G = L.MODEL_GMVAE
    h = C.c_void_p()
    GA, F, SL = L.LIK_GAUSSIAN, L.X_F32, L.LIK_SCALE_LEARNED
    mk = lambda S, f, K=10: L.make_dims(16, 784, 8, K, (64,), S=S, sched_flags=f)
    oks = []
    for M in (GA | F, GA | SL, GA | F | SL):
        oks += [(mk(1, M), G), (mk(3, M), G), (mk(1, M, 1), L.MODEL_VAE), (mk(2, M), L.MODEL_VAE_GMP), (mk(1, M | L.OPT_CLIP_NORM), G)]
    for d, model in oks:
        assert L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
        assert L.lib.gmvae_iw_bound_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
    cases = []
    for M in (F, SL, F | SL, F | L.LIK_GREY_BERNOULLI, SL | L.LIK_CONT_BERNOULLI, F | SL | L.LIK_GREY_BERNOULLI):      # without the Gaussian
        cases += [(mk(1, M), G), (mk(3, M, 1), L.MODEL_VAE), (mk(1, M | L.OPT_CLIP_NORM), L.MODEL_VAE_GMP)]
    for M in (GA | F, GA | SL, GA | F | SL):                                                     # what check_lik_dims refuses
        cases += [(mk(1, M | L.OBJ_MARGINAL_Y), G), (mk(2, M | L.OBJ_MARGINAL_Y_IW), G), (mk(2, M | L.GRAD_DREG, 1), L.MODEL_VAE),
                  (mk(1, M | L.GRAD_DREG | L.OBJ_MARGINAL_Y), G), (mk(1, M | L.OBJ_LABELS | L.OBJ_MARGINAL_Y), G),
                  (mk(1, M | L.OBJ_WEIGHTS), G), (mk(1, M | L.Y_TEMP_DEV), G), (mk(3, M | L.Y_STRAIGHT_THROUGH), G),
                  (mk(1, M | L.OBJ_PIXEL_MASK), G), (mk(2, M | L.OBJ_PIXEL_MASK, 1), L.MODEL_VAE)]
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
    for d, model in oks:
        if d.sched_flags & L.OPT_CLIP_NORM:
            continue
        assert L.lib.gmvae_train_graph_create_pipeline(C.byref(d), model, p, 100, p, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999,
                                                       1e-8, None, C.byref(h)) == -2
    for M in (GA | F, GA | SL, GA | F | SL):      # the evaluators that would score Bernoulli
        d = mk(2, M)
        r = C.byref(d)
        assert L.lib.gmvae_iw_bound_enum_y_workspace_bytes(r, G, C.byref(u64)) == -2
        assert L.lib.gmvae_posterior_y_workspace_bytes(r, G, C.byref(u64)) == -2
        assert L.lib.gmvae_posterior_component_workspace_bytes(r, L.MODEL_VAE_GMP, C.byref(u64)) == -2
        assert L.lib.gmvae_iw_bound_enum_y(r, G, p, p, 4, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_posterior_y(r, G, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_posterior_component(r, L.MODEL_VAE_GMP, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
    assert h.value is None
    # x 4-byte but not 16-byte aligned under GMVAE_X_F32: GMVAE_E_ALIGN (-4), before any launch; fine for bytes
    d = mk(1, GA | F)
    r = C.byref(d)
    E_ALIGN = -4
    assert L.lib.gmvae_step(r, G, p4, None, None, p, p, p, 0, 0, None, None) == E_ALIGN
    assert L.lib.gmvae_forward(r, G, p4, None, None, p, p, None, None, None, None, p, 0, 0, None) == E_ALIGN
    assert L.lib.gmvae_train_graph_create(r, G, p4, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, C.byref(C.c_void_p())) == E_ALIGN
    assert L.lib.gmvae_dp_graph_create(r, G, p4, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None, C.byref(C.c_void_p())) == E_ALIGN
    assert L.lib.gmvae_bench_loop(r, G, p4, p, p, p, p, p, p, 1, 0, C.byref(C.c_float()), None) == E_ALIGN
    assert L.lib.gmvae_iw_bound(r, G, p4, p, 4, None, None, p, p, 0, 0, None) == E_ALIGN


# ------------------------------------------------------------------------------------------ the Python surface
def test_check_real_valued(L):
    from gmvae_amd.engine import LIKELIHOOD_SCALES, check_real_valued
    assert LIKELIHOOD_SCALES == ("fixed", "learned")
    for lik in L.LIKELIHOODS:
        check_real_valued(lik)                                   # off: nothing to refuse
    check_real_valued("gaussian", True, "learned")
    check_real_valued("gaussian", False, "learned")
    check_real_valued("gaussian", True, "fixed")
    for lik in ("bernoulli", "grey_bernoulli", "continuous_bernoulli"):
        with pytest.raises(ValueError, match="real_valued"):
            check_real_valued(lik, True)
        with pytest.raises(ValueError, match="likelihood_scale"):
            check_real_valued(lik, False, "learned")
    with pytest.raises(ValueError, match="likelihood_scale must be one of"):
        check_real_valued("gaussian", False, "per_pixel")


def test_engine_refuses_before_it_needs_a_device(L):
    from gmvae_amd.engine import Engine
    with pytest.raises(ValueError, match="real_valued"):
        Engine("vae", 20, 2, 1, [8], real_valued=True)
    with pytest.raises(ValueError, match="likelihood_scale"):
        Engine("vae", 20, 2, 1, [8], likelihood="continuous_bernoulli", likelihood_scale="learned")
    with pytest.raises(ValueError, match="y_inference"):        # (the Gaussian's own refusals hold)
        Engine("gmvae", 20, 2, 3, [8], likelihood="gaussian", real_valued=True, y_inference="marginal")
    with pytest.raises(ValueError, match="pixel_mask"):
        Engine("vae", 20, 2, 1, [8], likelihood="gaussian", likelihood_scale="learned", pixel_mask=True)


def test_runner_flags(L, tmp_path):
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    d = run_gmvae.check_args(p, p.parse_args([]))
    assert not d.real_valued and d.likelihood_scale == "fixed" and d.data_npy is None and not d.standardize and not runners.real_valued(d)
    ga = "--likelihood=gaussian"
    ok = run_gmvae.check_args(p, p.parse_args([ga, "--real_valued", "--likelihood_scale=learned", "--standardize", "--iw_samples=7",
                                               "--n_samples=3", "--clip_norm=5"]))
    assert runners.real_valued(ok) and ok.likelihood_scale == "learned" and ok.data_dim == 784
    run_gmvae.check_args(p, p.parse_args([ga, "--likelihood_scale=learned"]))             # byte input with the learned scale
    x = np.random.default_rng(0).normal(size=(12, 37)).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "y.npy", np.arange(12) % 3)
    np.save(tmp_path / "bad.npy", np.zeros(5, np.float32))
    cfg = run_gmvae.check_args(p, p.parse_args([ga, "--real_valued", f"--data_npy={tmp_path / 'x.npy'}", f"--labels_npy={tmp_path / 'y.npy'}"]))
    assert cfg.data_dim == 37                                                             # (--data_dim follows the file)
    rows, lab = runners.real_rows(cfg)
    assert rows.dtype == np.float32 and np.array_equal(rows, x) and np.array_equal(lab, np.arange(12) % 3)
    rv = ["--real_valued", ga]
    for bad in (["--real_valued"], ["--real_valued", "--likelihood=continuous_bernoulli"], ["--likelihood_scale=learned"],
                ["--likelihood_scale=learned", "--likelihood=grey_bernoulli"], ["--likelihood_scale=per_pixel", ga],
                [ga, f"--data_npy={tmp_path / 'x.npy'}"], [ga, "--standardize"], rv + [f"--labels_npy={tmp_path / 'y.npy'}"],
                rv + [f"--data_npy={tmp_path / 'missing.npy'}"], rv + [f"--data_npy={tmp_path / 'bad.npy'}"],
                rv + ["--y_inference=marginal"], rv + ["--model=vae", "--grad_estimator=dreg"], rv + ["--kl_weight=0.5"],
                rv + ["--temperature=0.5"], rv + ["--y_estimator=straight_through"], rv + ["--iw_enum_samples=4"],
                rv + ["--posterior_samples=4"], rv + ["--missing_rate=0.5"],
                rv + ["--model=vae_gmp", "--mode=eval", "--component_posterior_samples=4"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    xs, ls = runners.synthetic_real(256, 20)
    assert xs.dtype == np.float32 and xs.shape == (256, 20) and ls.shape == (256,) and set(ls.tolist()) <= set(range(10))
    x2, l2 = runners.synthetic_real(256, 20)
    assert np.array_equal(xs, x2) and np.array_equal(ls, l2)
    # well separated: every row lies nearest to its own blob's mean
    means = np.stack([xs[ls == k].mean(axis=0) for k in range(10)])
    assert (np.argmin(((xs[:, None, :] - means[None]) ** 2).sum(axis=2), axis=1) == ls).all()
    mean, std = runners.standardize_stats(xs)
    z = runners._standardized(xs, (mean, std))
    assert z.dtype == np.float32 and np.abs(z.mean(axis=0)).max() < 1e-5 and np.abs(z.std(axis=0) - 1).max() < 1e-4


# ------------------------------------------------------------------------------------------------ the statement
def test_real_batch():
    x, rho = RR.real_batch(64, 100, seed=5)
    assert x.dtype == np.float32 and rho.dtype == np.float32 and x.shape == (64, 100) and rho.shape == (100,)
    assert 0.05 < (x == 0).mean() < 0.15 and np.isfinite(x).all()
    amax = np.abs(x).max(axis=0)
    assert (amax < 0.01).sum() == 25 and (amax > 20).sum() == 25
    assert rho.min() >= np.log(0.05) - 1e-6 and rho.max() <= np.log(5.0) + 1e-6 and rho.std() > 0.5
    x2, rho2 = RR.real_batch(64, 100, seed=5)
    assert np.array_equal(x, x2) and np.array_equal(rho, rho2)


@pytest.mark.parametrize("name", ["vae-gauss-sigma-small", "gmvae-s3-gauss", "vae_gmp-tanh-gauss", "gumbel-d99-gauss"])
def test_on_bytes_over_255_it_is_lik_refs_gaussian(name):
    """With x = bytes / 255 and a scalar sigma the statement reproduces lik_ref's Gaussian numbers to 1e-12."""
    model, d, p, flat, x, eps, u = LR.setup(name)
    s = LR.CASES[name].sigma
    Cl, gl = LR.loss_and_grads(model, d, p, x, eps, u, "gauss", s)
    Cr, gr = RR.loss_and_grads(model, d, p, LR.targets(x), eps, u, sigma=s)
    for k in ("loss", "nll", "kl", "nent", "sqerr", "nll_abs"):
        assert abs(Cr[k] - Cl[k]) <= 1e-12 * max(abs(Cl[k]), Cl["nll_abs"], 1.0), k
    assert np.abs(Cr["rows"] - Cl["rows"]).max() <= 1e-12 * max(np.abs(Cl["rows"]).max(), Cl["nll_abs"])
    assert np.abs(Cr["bound"] - Cl["bound"]).max() <= 1e-12 * max(np.abs(Cl["bound"]).max(), Cl["nll_abs"])
    for k in gl:
        assert np.abs(gr[k] - gl[k]).max() <= 1e-12 * max(np.abs(gl[k]).max(), 1.0), k
    assert not gr[RR.LOG_SIGMA].any()                           # (a fixed scale has no gradient)
    # the same scale as a constant rho: the same numbers, and now a gradient
    Cq, gq = RR.loss_and_grads(model, d, p, LR.targets(x), eps, u, rho=np.full(d.D, np.log(s)))
    assert abs(Cq["loss"] - Cr["loss"]) <= 1e-12 * max(abs(Cr["loss"]), Cr["nll_abs"]) and gq[RR.LOG_SIGMA].any()


@pytest.mark.parametrize("name", ["gmvae-s3", "vae_gmp-tanh", "vae-b1-d3"])
def test_rho_gradient_against_central_differences(name):
    """d loss / d rho_d in fp64 against (loss(rho + h e_d) - loss(rho - h e_d)) / 2h, and its closed form under S = 1:
    mean_b (1 - (lambda - t)^2 / sigma_d^2)."""
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, "learned")
    C0, g = RR.loss_and_grads(model, d, p32, t, eps, u, rho=rho)
    gr = g[RR.LOG_SIGMA]
    assert gr.shape == (d.D,) and np.isfinite(gr).all()
    h = 1e-6
    for j in sorted({0, d.D // 3, d.D // 2, d.D - 1}):
        e = np.zeros(d.D)
        e[j] = h
        lp = RR.loss_and_grads(model, d, p32, t, eps, u, rho=rho + e)[0]["loss"]
        lm = RR.loss_and_grads(model, d, p32, t, eps, u, rho=rho - e)[0]["loss"]
        fd = (lp - lm) / (2 * h)
        assert abs(fd - gr[j]) <= 1e-6 * max(abs(gr[j]), 1.0) + 1e-9 * abs(C0["loss"]) / h * 1e-6, (j, fd, gr[j])
    if d.S == 1:
        closed = (1.0 - (C0["lam"] - t) ** 2 * np.exp(-2.0 * rho)[None, :]).mean(axis=0)
        assert np.abs(closed - gr).max() <= 1e-12 * max(np.abs(gr).max(), 1.0)


@pytest.mark.parametrize("name,scale", RR.VARIANTS)
def test_case_statements_are_finite(name, scale):
    import torch
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, scale)
    c = RR.CASES[name]
    assert x.dtype == (np.uint8 if c.bytes_in else np.float32) and x.shape == (c.B, d.D)
    P0 = O.pack(model, d, p32, np.float32).shape[0]
    assert flat.shape[0] == P0 + (RR.pad4(d.D) if scale == "learned" else 0)
    Cc, g = RR.loss_and_grads(model, d, p32, t, eps, u, sigma=c.sigma, rho=rho)
    assert all(np.isfinite(Cc[k]) for k in ("loss", "nll", "kl", "nent", "sqerr", "nll_abs")) and np.isfinite(Cc["rows"]).all()
    assert all(np.isfinite(v).all() for v in g.values()) and (g[RR.LOG_SIGMA].any() == (scale == "learned"))
    # terms_in at float64 IS this forward; at float32 it measures the case's conditioning (the device tests' allowance)
    t64 = RR.terms_in(torch.float64, model, d, p32, t, eps, u, sigma=c.sigma, rho=rho)
    assert np.abs(t64["rows"] - Cc["rows"]).max() <= 1e-12 * max(np.abs(Cc["rows"]).max(), 1.0)
    for k in ("loss", "nll", "kl", "nent", "sqerr"):
        assert abs(t64[k] - Cc[k]) <= 1e-12 * max(abs(Cc[k]), Cc["nll_abs"], 1.0), k
    t32 = RR.terms_in(torch.float32, model, d, p32, t, eps, u, sigma=c.sigma, rho=rho)
    print(f"{name}-{scale}: torch fp32 vs fp64, max over rows: logpx {np.abs(t32['rows'] - t64['rows']).max(axis=0).tolist()}; "
          f"rel loss {abs(t32['loss'] - t64['loss']) / abs(t64['loss']):.2e} kl {abs(t32['kl'] - t64['kl']) / max(abs(t64['kl']), 1):.2e}")
    print(f"{name}-{scale}: loss {Cc['loss']:.6g} nll {Cc['nll']:.6g} nll_abs {Cc['nll_abs']:.6g} kl {Cc['kl']:.6g} sqerr {Cc['sqerr']:.6g}")


# ------------------------------------------------------------------------- rho's reduction beyond one row slab
def test_beyond_one_slab_cases_are_what_their_comments_say():
    """(slabs, rows of the last slab, rows per thread, column strips, columns of the last strip, vector path, NS, NSB) of each case,
    from liksig.hpp's slab rule and gmvae_hip.hip's num_splits (R / 256, at most 16; NSB = min(NS, num_splits(B)) under S > 1)."""
    ns = lambda n: min(max(n // 256, 1), 16)
    want = {"vae-r130": (3, 2, 4, 2, 36, True, 1, 1), "gmvae-r650": (11, 10, 4, 2, 35, False, 2, 1),
            "vae-r16450": (129, 66, 8, 2, 4, True, 16, 1)}
    assert set(want) == set(RR.BEYOND_ONE_SLAB)
    for name in RR.BEYOND_ONE_SLAB:
        c = RR.CASES[name]
        R, D, S = c.B * c.d.S, c.d.D, c.d.S
        rs = RR.liksig_slab_rows(R)
        slabs = (R + rs - 1) // rs
        NS = ns(R)
        got = (slabs, R - (slabs - 1) * rs, rs // RR.LSIG_ROW_LANES, (D + 63) // 64, D - (D - 1) // 64 * 64, D % 4 == 0, NS,
               min(NS, ns(c.B)) if S > 1 else NS)
        assert got == want[name], (name, got)
        assert (RR.liksig_slab_rows(16384), RR.liksig_slab_rows(16385)) == (64, 128)


@pytest.mark.parametrize("name", RR.BEYOND_ONE_SLAB)
def test_rho_reduction_in_the_kernels_order_in_fp32(name):
    """The reference alone: rho's reduction over the statement's g and row weights, evaluated in numpy float32 in the kernel's
    order (rows per lane, then the 16 lanes, then the slabs), sits within a quarter of the device gate -- 2.5e-5 of max |ref| --
    of the fp64 gradient; in float64 the same code IS the statement's gradient.  The fp64 statement itself takes well under a
    second at these sizes."""
    import time
    model, d, p32, flat, x, t, eps, u, rho = RR.setup(name, "learned")
    B = x.shape[0]
    t0 = time.perf_counter()
    Cc, g = RR.loss_and_grads(model, d, p32, t, eps, u, rho=rho)
    secs = time.perf_counter() - t0
    ref = g[RR.LOG_SIGMA]
    gm, rw = RR.rho_terms(Cc, t, rho, d.S)
    if d.S == 1:
        assert (rw == 1.0).all()
    else:
        assert rw.min() < 0.5 / d.S and rw.max() > 2.0 / d.S                # (the row weights are live)
    e64 = np.abs(RR.rho_reduction(gm, rw, rho, np.float64) / B - ref).max() / np.abs(ref).max()
    e32 = np.abs(RR.rho_reduction(gm, rw, rho, np.float32) / B - ref).max() / np.abs(ref).max()
    print(f"{name}: fp64 statement {secs:.3f} s; rho reduction in the kernel's order: fp64 err {e64:.2e}, fp32 err {e32:.2e} of max |ref| "
          f"{np.abs(ref).max():.4g}")
    assert secs < 1.0
    assert e64 <= 1e-10 and e32 <= 2.5e-5, (name, e64, e32)
