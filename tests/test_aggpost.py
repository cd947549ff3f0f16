"""gmvae_mixture_logpdf_* (include/gmvae_hip.h; csrc/aggpost.hpp) and Engine.aggregate_posterior on the device against the fp64
statement (tests/aggpost_ref.py): the kernel on six shapes and five regimes with per_dim on and off and with and without
owners, chunked feeding and bit-equality of two calls, the memory contract on guarded buffers, the Engine-level dict on five
models at Xavier and at sharp posteriors, the model and runner surface.

The gate is the project's own: |got - ref| <= 1e-4 max(1, |ref|) per output element; a mean over the queries, being a difference
of two such terms, is held to 1e-4 max(1, mean|own|, mean|agg|).  Every test prints its worst figure before it asserts."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import oracle as O
import aggpost_ref as R
from arena import Arena

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 2), (67, 130, 5), (64, 257, 64), (40, 300, 128), (33, 200, 8)]      # (M, C, L)
REGIMES = ["wide", "narrow", "saturated", "far", "neg_inf"]
CPO = 7                # components per owner of the owner cases: the GMVAE's layout (K components per example)


def _L():
    from gmvae_amd import _lib
    return _lib


def make_case(shape, regime):
    """fp32 (z [M, L], mu [C, L], sigma [C, L], logw [C], owner [M] int64) of a shape in a regime."""
    M, Cn, Lz = shape
    rng = np.random.default_rng(1000 * SHAPES.index(shape) + REGIMES.index(regime))
    mu = rng.normal(0, 1, (Cn, Lz))
    z = rng.normal(0, 1.2, (M, Lz))
    logw = np.log(rng.dirichlet(np.ones(Cn)))
    if regime == "wide":
        sigma = rng.uniform(0.3, 1.5, (Cn, Lz))
    elif regime == "narrow":
        sigma = rng.uniform(1e-3, 0.1, (Cn, Lz))
    elif regime == "saturated":                     # sigma log-uniform in [2e-9, 20]; queries drawn from the components themselves
        sigma = np.exp(rng.uniform(math.log(2e-9), math.log(20.0), (Cn, Lz)))
        c = np.arange(M) % Cn
        z = mu[c] + sigma[c] * rng.normal(0, 1, (M, Lz))
    elif regime == "far":                           # every query far from every component: log-densities around -4e7
        sigma = rng.uniform(0.009, 0.011, (Cn, Lz))
        z = z + 50.0
    else:                                           # some weights -inf, some -1e4
        sigma = rng.uniform(0.3, 1.5, (Cn, Lz))
        logw[rng.random(Cn) < 0.3] = -np.inf
        logw[rng.random(Cn) < 0.3] = -1e4
        logw[0] = -np.inf if Cn > 1 else logw[0]
    owner = rng.integers(0, (Cn + CPO - 1) // CPO, M).astype(np.int64)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(z), f(mu), f(sigma), f(logw), owner


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_kernel(z, mu, sigma, logw, per_dim, owner=None, cpo=CPO, log_norm=0.0, splits=None):
    """accumulate (one call, or one per (lo, hi) of splits) + finish: dict of numpy outputs (None where not asked for)."""
    L = _L()
    M, Lz = z.shape
    nb = C.c_uint64()
    assert L.lib.gmvae_mixture_logpdf_workspace_bytes(M, Lz, int(per_dim), C.byref(nb)) == 0
    ws = torch.zeros(nb.value // 8, dtype=torch.float64, device="cuda")
    zd, od = dev(z), (None if owner is None else dev(owner))
    for lo, hi in (splits or [(0, mu.shape[0])]):
        m_, s_, w_ = dev(mu[lo:hi]), dev(sigma[lo:hi]), dev(logw[lo:hi])
        rc = L.lib.gmvae_mixture_logpdf_accumulate(L.ptr(zd), M, Lz, L.ptr(m_), L.ptr(s_), L.ptr(w_), hi - lo, lo, cpo, L.ptr(od),
                                                   int(per_dim), L.ptr(ws), L.current_stream())
        assert rc == 0, rc
    joint = torch.empty(M, device="cuda")
    dim = torch.empty(M, Lz, device="cuda") if per_dim else None
    own = torch.empty(M, device="cuda") if owner is not None else None
    rc = L.lib.gmvae_mixture_logpdf_finish(M, Lz, int(per_dim), float(log_norm), L.ptr(joint), L.ptr(dim), L.ptr(own), L.ptr(ws),
                                           L.current_stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return dict(log_joint=n(joint), log_dim=n(dim), log_own=n(own))


def gate_err(got, ref):
    """max over the elements of |got - ref| / max(1, |ref|); inf unless got is -inf / +inf exactly where the reference is and
    finite elsewhere."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not (np.array_equal(got[~fin], ref[~fin]) and np.all(np.isfinite(got[fin]))):
        return math.inf
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()) if fin.any() else 0.0


def check_outputs(what, o, ref, per_dim, owners):
    errs = {"log_joint": gate_err(o["log_joint"], ref["log_joint"])}
    if per_dim:
        errs["log_dim"] = gate_err(o["log_dim"], ref["log_dim"])
    if owners:
        errs["log_own"] = gate_err(o["log_own"], ref["log_own"])
    print(what, "per_dim", per_dim, "owners", owners, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-4, (what, errs)
    return max(errs.values())


_REF = {}


def reference(shape, regime):
    if (shape, regime) not in _REF:
        z, mu, sigma, logw, owner = make_case(shape, regime)
        _REF[(shape, regime)] = R.mixture_logpdf(z, mu, sigma, logw, 0.25, CPO, owner)
    return _REF[(shape, regime)]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_the_fp64_statement(shape, regime):
    z, mu, sigma, logw, owner = make_case(shape, regime)
    ref = reference(shape, regime)
    if regime == "far" and shape[2] > 1:
        assert np.all(np.isfinite(ref["log_joint"])) and ref["log_joint"].max() < -1e7      # the empty-state case: finite, not -inf
    for per_dim in (True, False):
        for owners in (True, False):
            o = run_kernel(z, mu, sigma, logw, per_dim, owner if owners else None, log_norm=0.25)
            assert (o["log_dim"] is None) == (not per_dim) and (o["log_own"] is None) == (not owners)
            check_outputs(f"{shape} {regime}", o, ref, per_dim, owners)


def test_chunked_feeding_and_bit_equal_calls():
    shape = (64, 257, 64)
    for regime in ("wide", "saturated"):
        z, mu, sigma, logw, owner = make_case(shape, regime)
        ref = reference(shape, regime)
        whole = run_kernel(z, mu, sigma, logw, True, owner, log_norm=0.25)
        cuts = [0, 1, 8, 40, 41, 129, 200, 257]                          # seven uneven chunks; owners straddle the cuts
        parts = run_kernel(z, mu, sigma, logw, True, owner, log_norm=0.25, splits=list(zip(cuts[:-1], cuts[1:])))
        check_outputs(f"{regime} whole", whole, ref, True, True)
        check_outputs(f"{regime} seven chunks", parts, ref, True, True)
        again = run_kernel(z, mu, sigma, logw, True, owner, log_norm=0.25)
        again7 = run_kernel(z, mu, sigma, logw, True, owner, log_norm=0.25, splits=list(zip(cuts[:-1], cuts[1:])))
        for k in whole:
            assert np.array_equal(whole[k], again[k]) and np.array_equal(parts[k], again7[k]), k


def test_memory_contract_on_guarded_buffers():
    """The three calls on arena buffers (M = 67, L = 5, C = 130: no size is a multiple of a tile): accumulate changes the
    workspace alone, finish the outputs alone."""
    L = _L()
    shape = (67, 130, 5)
    M, Cn, Lz = shape
    z, mu, sigma, logw, owner = make_case(shape, "wide")
    ref = reference(shape, "wide")
    nb = C.c_uint64()
    assert L.lib.gmvae_mixture_logpdf_workspace_bytes(M, Lz, 1, C.byref(nb)) == 0
    ar = Arena("cuda", 8 << 20)
    bufs = {}
    for name, a in (("z", z), ("mu", mu), ("sigma", sigma), ("logw", logw), ("owner", owner)):
        bufs[name] = ar.place(name, a.nbytes, a.shape[-1] * a.itemsize if a.ndim > 1 else a.itemsize, False,
                              torch.int64 if a.dtype == np.int64 else torch.float32)
        bufs[name].copy_(torch.from_numpy(a.reshape(-1)))
    ws = ar.place("workspace", nb.value, 16, True, torch.float64)
    ws.zero_()
    joint = ar.place("log_joint", M * 4, 4, False, torch.float32)
    dim = ar.place("log_dim", M * Lz * 4, Lz * 4, False, torch.float32)
    own = ar.place("log_own", M * 4, 4, False, torch.float32)
    ar.snapshot()
    for lo, hi in ((0, 77), (77, 130)):
        rc = L.lib.gmvae_mixture_logpdf_accumulate(L.ptr(bufs["z"]), M, Lz, L.ptr(bufs["mu"][lo * Lz:]), L.ptr(bufs["sigma"][lo * Lz:]),
                                                   L.ptr(bufs["logw"][lo:]), hi - lo, lo, CPO, L.ptr(bufs["owner"]), 1, L.ptr(ws),
                                                   L.current_stream())
        assert rc == 0
    ar.check()
    ar.set_writable("workspace", False)
    for name in ("log_joint", "log_dim", "log_own"):
        ar.set_writable(name, True)
    ar.snapshot()
    assert L.lib.gmvae_mixture_logpdf_finish(M, Lz, 1, 0.25, L.ptr(joint), L.ptr(dim), L.ptr(own), L.ptr(ws), L.current_stream()) == 0
    ar.check()
    o = dict(log_joint=joint.cpu().numpy(), log_dim=dim.view(M, Lz).cpu().numpy(), log_own=own.cpu().numpy())
    check_outputs("arena", o, ref, True, True)
    # finish with no output asked for writes nothing at all
    for name in ("log_joint", "log_dim", "log_own"):
        ar.set_writable(name, False)
    ar.snapshot()
    assert L.lib.gmvae_mixture_logpdf_finish(M, Lz, 1, 0.25, None, None, None, L.ptr(ws), L.current_stream()) == 0
    ar.check()


# ------------------------------------------------------------------------------------------------ Engine.aggregate_posterior
MODELS = {
    "vae": ("vae", O.Dims(D=64, L=8, K=1, hidden=(32,))),
    "vae_gmp": ("vae_gmp", O.Dims(D=64, L=8, K=5, hidden=(32,))),
    "gmvae": ("gmvae", O.Dims(D=64, L=8, K=5, hidden=(32,))),
    "gmvae_h24x2": ("gmvae", O.Dims(D=100, L=5, K=5, hidden=(24, 24))),
    "gmvae_tanh": ("gmvae", O.Dims(D=64, L=8, K=5, hidden=(32,), act="tanh")),
}
N_EX, SEED, STEP = 48, 11, 3
PER_QUERY = ("log_q_zx", "log_q_z", "log_q_zd", "log_p_z", "log_p_zd")
MEANS = ("kl_avg", "mi", "kl_marginal", "tc")


SHARP_SIGMA_MIN = 1.0


def make_engine(name, sharp):
    """(engine, model id, dims, fp32 parameters as a dict, x uint8 [N_EX, D]); sharp: every encoder weight matrix scaled by 8.
    The sharp models carry sigma_min = SHARP_SIGMA_MIN.  Scaling both layers by 8 scales the heads' outputs by 64: the means
    spread over +-150 (+-730 on the two-layer model) and raw sigma over +-100, so without a floor sigma = softplus(-100) = 4e-44
    and the statement itself is rounding noise -- fed the Engine's fp32 z, its (z - mu) / sigma takes the 1e-7 rounding of z and
    of the fp32 encoder against sigma, and its log q(z | x) reads -1e100 and beyond (measured: |ref| up to 3e243; no evaluator can
    be held to that).  With the floor the posteriors are still sharp where it counts -- sigma = 1 against means +-150 apart: the
    statement's mi is ln 48 = 3.871 on four models and 3.846 on the fifth, and the far components sit at -1e3 to -1e5 -- and the
    statement's own sensitivity to an fp32 encoder (NumPy fp32 against fp64, same z) is at most 1.9e-5 max(1, |ref|) per element,
    a fifth of the gate (5.4e-5 at a floor of 0.5, 2.0e-4 at 0.25: over the gate on the two-layer model)."""
    from gmvae_amd.engine import Engine
    mname, d = MODELS[name]
    if sharp:
        d = dataclasses.replace(d, sigma_min=SHARP_SIGMA_MIN)
    model = O.MODEL_NAMES[mname]
    p = O.init_params(model, d, np.random.default_rng(5))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(6).normal(0, 0.3, p[k].shape)
        elif sharp and k.startswith("encoder") and k.endswith("/w"):
            p[k] = p[k] * 8.0
    flat = O.pack(model, d, p, np.float32)
    e = Engine(mname, d.D, d.L, d.K, list(d.hidden), sigma_min=d.sigma_min, raw_sigma_bias=d.raw_sigma_bias, hidden_act=d.act,
               random_seed=1)
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(flat[:e.P]))
    e.noise_seed, e.global_step = SEED, STEP
    x = (np.random.default_rng(7).random((N_EX, d.D)) < 0.5).astype(np.uint8)
    return e, model, d, O.unpack(model, d, flat), x


def check_dict(what, got, ref, n_examples, gm):
    """Everything but the means: the per-query outputs, the identity, the pointwise bound, the encoder-only statistics."""
    g = lambda k: got[k].double().cpu().numpy()
    errs = {k: gate_err(g(k), ref[k]) for k in PER_QUERY}
    scale = max(1.0, np.abs(ref["log_q_zx"]).mean(), np.abs(ref["log_q_z"]).mean())
    errs["identity"] = abs(g("kl_avg") - g("mi") - g("kl_marginal")) / scale
    errs["au_variance"] = gate_err(g("au_variance"), ref["au_variance"])
    if gm:
        errs["q_y"] = gate_err(g("q_y"), ref["q_y"])
        errs["q_y_entropy"] = abs(g("q_y_entropy") - ref["q_y_entropy"])
        errs["mi_xy"] = abs(g("mi_xy") - ref["mi_xy"])
    print(what, "scale", f"{scale:.3g}", {k: f"{float(v):.2e}" for k, v in errs.items()})
    assert max(float(v) for v in errs.values()) <= 1e-4, (what, errs)
    over = (g("log_q_zx") - g("log_q_z") - math.log(n_examples)) / np.maximum(1.0, np.abs(ref["log_q_zx"]))
    assert over.max() <= 1e-4, over.max()                              # pointwise own - agg <= ln N (plus the gate)
    assert int(got["active_units"]) == ref["active_units"] or np.abs(ref["au_variance"] - 0.01).min() < 1e-5
    if not gm:
        assert got["q_y"] is None and got["q_y_entropy"] is None and got["mi_xy"] is None


def mean_errs(what, got, ref):
    """|err| / max(1, mean|own|, mean|agg|) of every mean over the queries."""
    g = lambda k: got[k].double().cpu().numpy()
    scale = max(1.0, np.abs(ref["log_q_zx"]).mean(), np.abs(ref["log_q_z"]).mean())
    errs = {k: float(abs(g(k) - ref[k]) / scale) for k in MEANS}
    errs["dim_kl"] = float(np.abs(g("dim_kl") - ref["dim_kl"]).max() / scale)
    print(what, "scale", f"{scale:.3g}", "mean|log_p_z|", f"{np.abs(ref['log_p_z']).mean():.3g}", {k: f"{v:.2e}" for k, v in errs.items()})
    return errs


SUBSET = np.array([5, 0, 47, 5, 20, 33, 1], np.int64)
CASES = [("all", None, 0, None), ("subset chunk 7", SUBSET, 13, 7)]      # (what, queries, row0, chunk)


@pytest.mark.parametrize("sharp", [False, True], ids=["xavier", "sharp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_matches_the_statement(name, sharp):
    e, model, d, p, x = make_engine(name, sharp)
    gm = model == O.MODEL_GMVAE
    xd = torch.from_numpy(x).cuda()
    comps = R.components(model, d, p, x)
    for what, qidx, row0, chunk in CASES:
        got = e.aggregate_posterior(xd, queries=None if qidx is None else torch.from_numpy(qidx), chunk=chunk, row0=row0)
        q = np.arange(N_EX) if qidx is None else qidx
        z_ref, k_ref = R.sample(model, d, comps, q, row0, SEED, STEP)
        z = got["z"].cpu().numpy()
        zerr = gate_err(z, z_ref)
        print(name, what, "z", f"{zerr:.2e}", "k", np.bincount(k_ref, minlength=d.K))
        assert zerr <= 1e-4
        check_dict(f"{name} sharp={sharp} {what}", got, R.statement(model, d, p, x, q, z), N_EX, gm)
    # the chunk changes nothing but the order of the fp64 folds (and the encoders' batch): chunk = 7 against chunk = N
    a, b = e.aggregate_posterior(xd, chunk=7), e.aggregate_posterior(xd, chunk=N_EX)
    ref = R.statement(model, d, p, x, np.arange(N_EX), b["z"].cpu().numpy())
    assert gate_err(a["z"].cpu().numpy(), b["z"].cpu().numpy()) <= 1e-4
    check_dict(f"{name} sharp={sharp} chunk 7 against the statement at chunk N's z", a, ref, N_EX, gm)
    # per_dim=False: the same joint terms, no per-dimension ones
    c = e.aggregate_posterior(xd, per_dim=False, chunk=N_EX)
    assert c["log_q_zd"] is None and c["log_p_zd"] is None and c["tc"] is None and c["dim_kl"] is None
    for k in ("z", "log_q_zx", "log_q_z"):
        assert torch.equal(c[k], b[k]), k
    # one example: q(z) = q(z | x), mi = 0
    one = e.aggregate_posterior(xd[:1])
    scale = max(1.0, abs(one["log_q_zx"].item()))
    print(name, "N = 1: mi", one["mi"].item(), "scale", scale)
    assert abs(one["mi"].item()) <= 1e-4 * scale


@pytest.mark.parametrize("sharp", [False, True], ids=["xavier", "sharp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_means_meet_the_gate(name, sharp):
    """Every mean over the queries within 1e-4 max(1, mean|own|, mean|agg|) of the statement's, over all 48 queries at chunk = N
    and at chunk = 7.  The 7-query subset's means are printed, not gated: its per-query outputs are gated in
    test_engine_matches_the_statement, and on gmvae_h24x2-sharp no fp32 evaluator can bring a mean of 7 inside this bound.
    Scaling both hidden layers and the head by 8 puts z at +-700 prior standard deviations there, so log p(z) is -1e5 on
    average (-3.5e5 at most) while own and agg are about 25; kl_avg, kl_marginal and dim_kl subtract that prior term, and half
    an fp32 ulp of ONE such log p(z) (0.016) is 6 times the bound (1e-4 x 25).  Measured on the MI355X on that model: all 48
    queries kl_avg 8.9e-5, dim_kl 3.5e-5 (inside: the roundings average out); the subset kl_avg 4.8e-4, kl_marginal 4.8e-4,
    dim_kl 5.5e-4; mi and tc, which do not touch the prior, 2e-9 to 6e-7.  The other nine cases, subset included, are at 2e-5
    and below."""
    e, model, d, p, x = make_engine(name, sharp)
    xd = torch.from_numpy(x).cuda()
    for what, qidx, row0, chunk in CASES + [("all chunk 7", None, 0, 7)]:
        got = e.aggregate_posterior(xd, queries=None if qidx is None else torch.from_numpy(qidx), chunk=chunk, row0=row0)
        q = np.arange(N_EX) if qidx is None else qidx
        errs = mean_errs(f"{name} sharp={sharp} {what}", got, R.statement(model, d, p, x, q, got["z"].cpu().numpy()))
        if qidx is None:
            assert max(errs.values()) <= 1e-4, (what, errs)


KEYS = {"z", "log_q_zx", "log_q_z", "log_q_zd", "log_p_z", "log_p_zd", "kl_avg", "mi", "kl_marginal", "tc", "dim_kl",
        "au_variance", "active_units", "q_y", "q_y_entropy", "mi_xy"}


def test_model_surface_and_refusals():
    from gmvae_amd.engine import Engine
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    x = torch.from_numpy((np.random.default_rng(2).random((24, 64)) < 0.5).astype(np.uint8)).cuda()
    for model in (create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1),
                  create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1),
                  create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)):
        o = model.latent_diagnostics(x)
        assert set(o) == KEYS and o["z"].shape == (24, 4) and o["log_q_zd"].shape == (24, 4) and o["dim_kl"].shape == (4,)
        assert all(torch.isfinite(o[k]).all() for k in PER_QUERY + MEANS)
        assert o["mi"].item() <= math.log(24) + 1e-4
        q = model.latent_diagnostics(x, queries=torch.tensor([3, 3, 9]), per_dim=False)
        assert q["z"].shape == (3, 4) and q["log_q_zd"] is None and q["log_q_z"].shape == (3,)
        with pytest.raises(ValueError, match="queries"):
            model.latent_diagnostics(x, queries=torch.tensor([24]))
        with pytest.raises(ValueError, match="chunk"):
            model._engine.aggregate_posterior(x, chunk=0)
    with pytest.raises(ValueError, match="pixel_mask"):
        Engine("vae", 64, 4, 1, [16], pixel_mask=True, random_seed=1).aggregate_posterior(x)


@pytest.mark.parametrize("model", ["gmvae", "vae_gmp"])
def test_run_eval_reports_the_diagnostics(tmp_path, model):
    from gmvae_amd import run_gmvae
    args = [f"--model={model}", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200", "--batch_size=40"]
    run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--latent_diagnostics=64"] + args)
    new = {f"train/{k}" for k in ("mi_xz", "kl_marginal", "total_correlation", "kl_avg", "active_units")}
    if model == "gmvae":
        new |= {"train/mi_xy", "train/q_y_entropy"}
    for k in new:
        print(k, res[k])
        assert math.isfinite(res[k]), k
    assert res["train/mi_xz"] <= math.log(64) + 1e-4
    assert res["train/kl_avg"] == pytest.approx(res["train/mi_xz"] + res["train/kl_marginal"], abs=1e-4 * max(1.0, abs(res["train/kl_avg"])))
    plain = run_gmvae.main(["--mode=eval"] + args)
    assert set(plain) == set(res) - new and not new & set(plain)
