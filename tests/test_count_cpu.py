"""Count data under the Poisson and the negative-binomial decoder (GMVAE_LIK_POISSON, GMVAE_LIK_NEG_BINOMIAL) without a device: the
anchors of the fp64 statement (tests/count_ref.py) -- torch.distributions with fp64 autograd, known values of digamma and of the
lgamma difference --, base.Poisson / base.NegativeBinomial, the library's flag values / schedule names / parameter layout /
workspace / refusals, and the Python and runner argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import count_ref as CR
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def r256(n):
    return (n + 255) // 256 * 256


def _elements(seed=0, n=400):
    rng = np.random.default_rng(seed)
    x = np.floor(np.exp(rng.uniform(0, 8, n)))
    x[::5] = 0.0
    x[1::7] += 0.5                                    # (nothing assumes integers)
    return x, rng.uniform(-12, 12, n), rng.uniform(-5, 8, n)


# ------------------------------------------------------------------------------------------------ the statement
def test_statement_against_torch_distributions():
    """log p, g = d(-log p)/d lambda and d log p / d rho of count_ref against torch.distributions.Poisson / NegativeBinomial
    (total_count = r, logits = lambda - rho) with fp64 autograd."""
    x, lam, rho = _elements()
    xt = torch.tensor(x)
    lt = torch.tensor(lam, requires_grad=True)
    lp = torch.distributions.Poisson(torch.exp(lt), validate_args=False).log_prob(xt)
    lp.sum().backward()
    assert np.allclose(CR.log_prob("poisson", x, lam), lp.detach().numpy(), rtol=1e-12, atol=1e-9)
    assert np.allclose(CR.grad_logit("poisson", x, lam), -lt.grad.numpy(), rtol=1e-12, atol=1e-12)
    xi = np.floor(x)                                  # (torch's NegativeBinomial validates integer support)
    lt = torch.tensor(lam, requires_grad=True)
    rt = torch.tensor(rho, requires_grad=True)
    nb = torch.distributions.NegativeBinomial(total_count=torch.exp(rt), logits=lt - rt, validate_args=False)
    lp = nb.log_prob(torch.tensor(xi))
    lp.sum().backward()
    ref = lp.detach().numpy()
    assert np.abs(CR.log_prob("nb", xi, lam, rho) - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1.0)
    g, gr = -lt.grad.numpy(), rt.grad.numpy()
    assert np.abs(CR.grad_logit("nb", xi, lam, rho) - g).max() <= 1e-10 * np.abs(g).max()
    assert np.abs(CR.grad_rho(xi, lam, rho) - gr).max() <= 1e-9 * np.abs(gr).max()
    assert np.allclose(nb.mean.detach().numpy(), np.exp(lam), rtol=1e-10)


def test_digamma_and_lgamma_difference_known_answers():
    tol = 2.0 / (12 * 6.0 ** 14)                      # (the series' first dropped term at the argument 6 where it starts: 1e-12)
    assert abs(CR.digamma(1.0) + CR.EULER_GAMMA) < tol
    assert abs(CR.digamma(0.5) + CR.EULER_GAMMA + 2 * math.log(2.0)) < tol
    v = np.exp(np.linspace(math.log(1e-3), math.log(1e5), 300))
    assert np.abs((CR.digamma(v + 1.0) - CR.digamma(v)) * v - 1.0).max() < 1e-9      # psi(v + 1) - psi(v) = 1 / v
    ref = torch.digamma(torch.tensor(v)).numpy()
    assert np.abs(CR.digamma(v) - ref).max() < tol
    for r in (math.exp(-5.0), 1.0, 2.5, math.exp(8.0)):
        for n in (0, 1, 2, 7, 100):
            want = sum(math.log(r + i) for i in range(n))                            # integer x: sum_i log(r + i)
            assert abs(CR.lgamma_diff(float(n), r) - want) <= 1e-11 * max(abs(want), 1.0), (r, n)
    assert CR.lgamma_diff(0.0, 1e-3) == 0.0


def test_whole_step_statement_matches_the_elementwise_one():
    """The adapter onto objective_ref: its log p(x|z) rows, its rho gradient and tail[5] are the NumPy statement's on the same
    lambda, with the row weights of the importance-weighted bound."""
    for name, kind in (("vae-b5-d13-s3", "poisson"), ("gmvae-b5-d100-s1", "nb"), ("vae_gmp-b5-d128-s3", "nb")):
        model, d, p32, flat, x, eps, u, rho = CR.setup(name, kind)
        Cc, g = CR.loss_and_grads(model, d, p32, x, eps, u, kind, rho)
        B, S = x.shape[0], d.S
        xr = np.repeat(x.astype(np.float64), S, axis=0)
        assert np.allclose(CR.log_prob(kind, xr, Cc["lam"], rho).sum(axis=1), Cc["rows"][:, 0], rtol=1e-12, atol=1e-9)
        assert np.isfinite(Cc["loss"]) and Cc["sqerr"] > 0 and Cc["nll_abs"] > 0
        if kind == "nb":
            rw = CR.row_weights(Cc, S)
            want = -(rw[:, None] * CR.grad_rho(xr, Cc["lam"], rho)).sum(axis=0) / B
            assert np.abs(want - g[CR.LOG_DISPERSION]).max() <= 1e-10 * np.abs(want).max()
        else:
            assert not g[CR.LOG_DISPERSION].any()


def test_batches_and_cases():
    x, rho = CR.count_batch(32, 100)
    assert x.dtype == np.float32 and (x >= 0).all() and (x == np.floor(x)).all() and (x == 0).mean() > 0.2 and x.max() >= 100
    xs, rs = CR.saturated_batch(32, 100)
    assert xs.max() == 1e4 and (xs == 0).mean() > 0.2 and set(rs.tolist()) == {-5.0, 0.0, 8.0}
    assert len(CR.CASES) == 18 and {c.B for c in CR.CASES.values()} == {32, 5}
    assert {c.d.D for c in CR.CASES.values()} == {128, 100, 13} and {c.d.S for c in CR.CASES.values()} == {1, 3}
    for B in (32, 5):
        assert {S for b, D, S in CR.SHAPES if b == B} == {1, 3}
    model, d, p32, flat, x, eps, u, rho = CR.setup("gmvae-b32-d100-s3", "nb", saturated=True)
    lam = CR.loss_and_grads(model, d, p32, x, eps, u, "nb", rho)[0]["lam"]
    assert 20 < np.abs(lam).max() < 40 and lam.min() < -10 and lam.max() > 10


# ------------------------------------------------------------------------------------------------ base
def test_base_distributions_against_torch():
    from gmvae_amd import base
    x, lam, rho = _elements(3, 60)
    x = np.floor(x)
    xt, lt, rt = (torch.tensor(a.reshape(6, 10)) for a in (x, lam, rho))
    P = base.Poisson(lt)
    assert torch.allclose(P.log_prob(xt), torch.distributions.Poisson(torch.exp(lt)).log_prob(xt).sum(-1), rtol=1e-12)
    assert torch.equal(P.mean(), torch.exp(lt))
    N = base.NegativeBinomial(lt, rt[0])
    ref = torch.distributions.NegativeBinomial(total_count=torch.exp(rt[0]), logits=lt - rt[0], validate_args=False)
    assert torch.allclose(N.log_prob(xt), ref.log_prob(xt).sum(-1), rtol=1e-10)
    assert torch.equal(N.mean(), torch.exp(lt))
    s = base.NegativeBinomial(torch.zeros(4000, 2, dtype=torch.float64) + 1.0, torch.zeros(2, dtype=torch.float64)).sample(seed=1)
    assert bool((s >= 0).all()) and abs(s.mean().item() - math.e) < 0.3 and s.var().item() > 1.5 * math.e      # over-dispersed
    assert abs(base.Poisson(torch.zeros(4000, 2, dtype=torch.float64) + 1.0).sample(seed=1).mean().item() - math.e) < 0.2


# ------------------------------------------------------------------------------------------------ the library
def test_flag_values_header_text_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    for name, val in (("GMVAE_LIK_POISSON", 1 << 15), ("GMVAE_LIK_NEG_BINOMIAL", 1 << 16)):
        m = re.search(name + r"\s*=\s*(\d+)\s*<<\s*(\d+)", hdr)
        assert m and int(m.group(1)) << int(m.group(2)) == val, name
    assert (L.LIK_POISSON, L.LIK_NEG_BINOMIAL) == (CR.LIK_POISSON, CR.LIK_NEG_BINOMIAL) == (1 << 15, 1 << 16)
    assert L.X_F32 == CR.X_F32 and L.LOG_DISPERSION == CR.LOG_DISPERSION == "decoder/log_dispersion"
    assert L.COUNT_LIKELIHOODS == {"poisson": L.LIK_POISSON, "negative_binomial": L.LIK_NEG_BINOMIAL}
    others = (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG | L.OBJ_LABELS |
              L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH | L.OBJ_PIXEL_MASK | L.OPT_CLIP_NORM | L.LIK_MASK | L.X_F32 |
              L.LIK_SCALE_LEARNED)
    assert (L.LIK_POISSON | L.LIK_NEG_BINOMIAL) & others == 0 and L.LIK_POISSON != L.LIK_NEG_BINOMIAL
    for text in ("decoder/log_dispersion", "log1p(x_bd)", '"+pois"', '"+nb"', "psi = digamma", "general+nb+f32+clip"):
        assert text in hdr, text
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


def test_schedule_names(L):
    F = L.X_F32
    for mk, model in ((lambda fl: L.make_dims(1024, 784, 64, 10, (64,), sched_flags=fl), L.MODEL_GMVAE),
                      (lambda fl: L.make_dims(25600, 3072, 128, 64, (512, 512), sched_flags=fl), L.MODEL_GMVAE),
                      (lambda fl: L.make_dims(1024, 784, 2, 1, (64,), sched_flags=fl), L.MODEL_VAE),
                      (lambda fl: L.make_dims(8, 96, 4, 6, (16,), S=3, sched_flags=fl), L.MODEL_VAE_GMP)):
        assert L.step_schedule(mk(L.LIK_POISSON | F), model) == "general+pois+f32"
        assert L.step_schedule(mk(L.LIK_NEG_BINOMIAL | F), model) == "general+nb+f32"
        assert L.step_schedule(mk(L.LIK_NEG_BINOMIAL | F | L.OPT_CLIP_NORM), model) == "general+nb+f32+clip"
        assert L.step_schedule(mk(L.LIK_GAUSSIAN | F), model) == "general+gauss+f32"      # (untouched)


@pytest.mark.parametrize("case", [("gmvae", 5, 99, 5, 7, (24,)), ("vae", 1, 3, 2, 1, (8,)), ("vae_gmp", 9, 100, 5, 3, (24,))],
                         ids=lambda c: f"{c[0]}-D{c[2]}")
def test_parameter_layout_and_workspace(L, case):
    """rho comes last under the negative binomial alone, in log_sigma's slot: P grows by pad4(D); the Poisson's layout is the
    plain one.  The workspace grows behind the plain step's by t [B D], the squared-error partials, c [B] -- and under the
    negative binomial sp(u) [R D] and the fp64 slab partials --, each rounded up to 256 bytes."""
    mname, B, D, Lz, K, hidden = case
    model = L.MODEL_IDS[mname]
    mk = lambda fl, S=1: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=fl)
    P0, lay0 = L.param_count(mk(0), model)[0], L.param_layout(mk(0), model)
    Pp, layp = L.param_count(mk(L.LIK_POISSON | L.X_F32), model)[0], L.param_layout(mk(L.LIK_POISSON | L.X_F32), model)
    Pn, layn = L.param_count(mk(L.LIK_NEG_BINOMIAL | L.X_F32), model)[0], L.param_layout(mk(L.LIK_NEG_BINOMIAL | L.X_F32), model)
    Pg = L.param_count(mk(L.LIK_GAUSSIAN | L.X_F32 | L.LIK_SCALE_LEARNED), model)[0]
    assert (Pp, layp) == (P0, lay0) and Pn == P0 + CR.pad4(D) == Pg
    assert layn[:-1] == lay0 and layn[-1][0] == "decoder/log_dispersion" and tuple(layn[-1][1]) == (1, D) and layn[-1][2] == P0
    for S in (1, 3):
        R = B * S
        w0 = L.workspace_bytes(mk(0, S), model)
        common = r256(4 * B * D) + r256(4 * R * ((D + 31) // 32)) + r256(4 * B)
        assert L.workspace_bytes(mk(L.LIK_POISSON | L.X_F32, S), model) == w0 + common
        slabs = (R + 63) // 64
        extra = r256(4 * R * D) + r256(8 * slabs * CR.pad4(D))
        wn = L.workspace_bytes(mk(L.LIK_NEG_BINOMIAL | L.X_F32, S), model)
        # (the split-K slabs of the gradient grow with P: compare against the learned Gaussian's workspace, whose P is the same)
        wg = L.workspace_bytes(mk(L.LIK_GAUSSIAN | L.X_F32 | L.LIK_SCALE_LEARNED, S), model)
        assert wn - wg == r256(4 * B * D) + r256(4 * B) + extra - r256(4 * slabs * CR.pad4(D))


def refusals(L):
    """GMVAE_E_DIMS from every entry that sizes or runs a step, before anything is touched (every pointer is a host dummy): a
    count bit without GMVAE_X_F32, beside the GMVAE_LIK_* field, beside GMVAE_LIK_SCALE_LEARNED, both bits at once, every
    objective bit but clip_norm, the pipeline graph and every evaluator but gmvae_iw_bound; GMVAE_E_ALIGN for an unaligned x."""
    u64 = C.c_uint64()
    buf = C.create_string_buffer(4096 + 16)
    base = (C.addressof(buf) + 15) // 16 * 16
    p, p4 = C.c_void_p(base), C.c_void_p(base + 4)
    G = L.MODEL_GMVAE
    h = C.c_void_p()
    F, PO, NB = L.X_F32, L.LIK_POISSON, L.LIK_NEG_BINOMIAL
    mk = lambda S, f, K=10: L.make_dims(16, 784, 8, K, (64,), S=S, sched_flags=f)
    oks = []
    for M in (PO | F, NB | F):
        oks += [(mk(1, M), G), (mk(3, M), G), (mk(1, M, 1), L.MODEL_VAE), (mk(2, M), L.MODEL_VAE_GMP), (mk(1, M | L.OPT_CLIP_NORM), G)]
    for d, model in oks:
        assert L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
        assert L.lib.gmvae_iw_bound_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
    cases = []
    for M in (PO, NB, PO | NB | F, PO | F | L.LIK_GAUSSIAN, NB | F | L.LIK_GREY_BERNOULLI, NB | F | L.LIK_CONT_BERNOULLI,
              PO | F | L.LIK_SCALE_LEARNED, NB | F | L.LIK_SCALE_LEARNED, NB | F | L.LIK_GAUSSIAN | L.LIK_SCALE_LEARNED):
        cases += [(mk(1, M), G), (mk(3, M, 1), L.MODEL_VAE), (mk(1, M | L.OPT_CLIP_NORM), L.MODEL_VAE_GMP)]
    for M in (PO | F, NB | F):
        cases += [(mk(1, M | L.OBJ_MARGINAL_Y), G), (mk(2, M | L.OBJ_MARGINAL_Y_IW), G), (mk(2, M | L.GRAD_DREG, 1), L.MODEL_VAE),
                  (mk(1, M | L.OBJ_LABELS | L.OBJ_MARGINAL_Y), G), (mk(1, M | L.OBJ_WEIGHTS), G), (mk(1, M | L.Y_TEMP_DEV), G),
                  (mk(3, M | L.Y_STRAIGHT_THROUGH), G), (mk(1, M | L.OBJ_PIXEL_MASK), G), (mk(2, M | L.OBJ_PIXEL_MASK, 1), L.MODEL_VAE)]
    for d, model in cases:
        r = C.byref(d)
        assert L.lib.gmvae_workspace_bytes(r, model, C.byref(u64)) == -2
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
    for M in (PO | F, NB | F):      # the evaluators that would score Bernoulli: the new bits pass "the LIK field != 0" tests
        d = mk(2, M)
        r = C.byref(d)
        V = L.MODEL_VAE_GMP
        assert L.lib.gmvae_iw_bound_enum_y_workspace_bytes(r, G, C.byref(u64)) == -2
        assert L.lib.gmvae_posterior_y_workspace_bytes(r, G, C.byref(u64)) == -2
        assert L.lib.gmvae_posterior_component_workspace_bytes(r, V, C.byref(u64)) == -2
        assert L.lib.gmvae_iw_bound_enum_y(r, G, p, p, 4, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_posterior_y(r, G, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_posterior_component(r, V, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
        assert L.lib.gmvae_impute_workspace_bytes(r, G, 0, C.byref(u64)) == -2
        assert L.lib.gmvae_impute(r, G, p, p, 4, 0, p, p, None, None, None, p, p, 0, 0, None) == -2
        d1 = mk(1, M)
        r1 = C.byref(d1)
        assert L.lib.gmvae_ais_workspace_bytes(r1, G, 0, 2, C.byref(u64)) == -2
        assert L.lib.gmvae_ais_reverse_workspace_bytes(r1, G, 0, 2, C.byref(u64)) == -2
        assert L.lib.gmvae_simulate_workspace_bytes(r1, G, C.byref(u64)) == -2
        assert L.lib.gmvae_refine_workspace_bytes(r1, G, 4, C.byref(u64)) == -2
        assert L.lib.gmvae_simulate(r1, G, p, None, None, None, p, p, p, p, p, 0, 0, None) == -2
    assert h.value is None
    E_ALIGN = -4
    for M in (PO | F, NB | F):
        d = mk(1, M)
        r = C.byref(d)
        assert L.lib.gmvae_step(r, G, p4, None, None, p, p, p, 0, 0, None, None) == E_ALIGN
        assert L.lib.gmvae_forward(r, G, p4, None, None, p, p, None, None, None, None, p, 0, 0, None) == E_ALIGN
        assert L.lib.gmvae_train_graph_create(r, G, p4, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, C.byref(C.c_void_p())) == E_ALIGN
        assert L.lib.gmvae_iw_bound(r, G, p4, p, 4, None, None, p, p, 0, 0, None) == E_ALIGN


def test_refusals_by_code(L):
    refusals(L)


# ------------------------------------------------------------------------------------------ the Python surface
def test_engine_argument_checks(L):
    from gmvae_amd.engine import Engine, check_count_likelihood, check_real_valued
    for lik in ("poisson", "negative_binomial"):
        check_real_valued(lik)                                   # implied
        check_real_valued(lik, True)
        with pytest.raises(ValueError, match="real_valued=False"):
            check_real_valued(lik, False)
        with pytest.raises(ValueError, match="likelihood_scale"):
            check_real_valued(lik, None, "learned")
        check_count_likelihood("gmvae", "gumbel", "standard", False, False, False, "relaxed", False, lik)
        with pytest.raises(ValueError, match="y_inference"):
            check_count_likelihood("gmvae", "marginal", "standard", False, False, False, "relaxed", False, lik)
        with pytest.raises(ValueError, match="pixel_mask"):
            check_count_likelihood("vae", "gumbel", "standard", False, False, False, "relaxed", True, lik)
        with pytest.raises(ValueError, match="real_valued=False"):
            Engine("vae", 20, 2, 1, [8], likelihood=lik, real_valued=False)
        with pytest.raises(ValueError, match="dreg"):
            Engine("vae", 20, 2, 1, [8], likelihood=lik, grad_estimator="dreg", n_samples=2)
    with pytest.raises(ValueError, match="likelihood must be one of"):
        check_count_likelihood("vae", "gumbel", "standard", False, False, False, "relaxed", False, "zero_inflated")
    with pytest.raises(ValueError, match="likelihood must be one of"):
        Engine("vae", 20, 2, 1, [8], likelihood="zero_inflated")


def test_runner_flags(L, tmp_path):
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    x = np.random.default_rng(0).poisson(3.0, (12, 37)).astype(np.float32)
    np.save(tmp_path / "x.npy", x)
    np.save(tmp_path / "y.npy", np.arange(12) % 3)
    data = f"--data_npy={tmp_path / 'x.npy'}"
    for lik in ("poisson", "negative_binomial"):
        cfg = run_gmvae.check_args(p, p.parse_args([f"--likelihood={lik}", data, "--iw_samples=7", "--clip_norm=5"]))
        assert cfg.likelihood == lik and cfg.real_valued and runners.real_valued(cfg) and runners.count_data(cfg)
        assert runners.likelihood_of(cfg)[0] == lik and cfg.data_dim == 37
        with pytest.raises(SystemExit):                                  # (counts come from a file)
            run_gmvae.check_args(p, p.parse_args([f"--likelihood={lik}"]))
        for bad in (["--standardize"], ["--y_inference=marginal"], ["--missing_rate=0.5"], ["--iw_enum_samples=4"],
                    ["--posterior_samples=4"], ["--likelihood_scale=learned"], ["--kl_weight=0.5"]):
            with pytest.raises(SystemExit):
                run_gmvae.check_args(p, p.parse_args([f"--likelihood={lik}", data] + bad))
    assert not runners.count_data(run_gmvae.check_args(p, p.parse_args([])))
    cfg = run_gmvae.check_args(p, p.parse_args(["--likelihood=negative_binomial", f"--data_npy={tmp_path / 'x.npy'}",
                                               f"--labels_npy={tmp_path / 'y.npy'}"]))
    assert cfg.data_dim == 37
    rows, lab = runners.real_rows(cfg)
    assert np.array_equal(rows, x) and np.array_equal(lab, np.arange(12) % 3)
    for badv in (-1.0, np.nan, np.inf):                                  # refused once, where the rows are loaded
        y = x.copy()
        y[3, 4] = badv
        np.save(tmp_path / "bad.npy", y)
        cfg = run_gmvae.check_args(p, p.parse_args(["--likelihood=poisson", f"--data_npy={tmp_path / 'bad.npy'}"]))
        with pytest.raises(ValueError, match="count data"):
            runners.real_rows(cfg)
    import types
    cfg = types.SimpleNamespace(likelihood="poisson", synthetic_size=64, data_dim=20, mixture_components=3, data_npy=None)
    rows, lab = runners.real_rows(cfg)                                   # (a config without a file: the synthetic stand-in)
    assert rows.shape == (64, 20) and np.array_equal(rows, runners.synthetic_counts(64, 20, 3)[0])


def test_synthetic_counts_is_reproducible():
    from gmvae_amd import runners
    x, lab = runners.synthetic_counts(512, 100, 3)
    x2, l2 = runners.synthetic_counts(512, 100, 3)
    assert np.array_equal(x, x2) and np.array_equal(lab, l2)
    assert x.dtype == np.float32 and x.shape == (512, 100) and lab.dtype == np.int64 and set(lab.tolist()) == {0, 1, 2}
    assert (x >= 0).all() and (x == np.floor(x)).all() and (x == 0).mean() > 0.1
    assert (x.var(axis=0) > 1.2 * x.mean(axis=0)).mean() > 0.8           # over-dispersed: not Poisson
    # the clusters are separable on the scale the networks read: nearest cluster mean of log1p(x) finds most labels
    t = np.log1p(x)
    means = np.stack([t[lab == k].mean(axis=0) for k in range(3)])
    assert (np.argmin(((t[:, None, :] - means[None]) ** 2).sum(axis=2), axis=1) == lab).mean() > 0.9
    assert not np.array_equal(x, runners.synthetic_counts(512, 100, 3, seed=8)[0])
