"""The weighted objective (GMVAE_OBJ_WEIGHTS) without a device: the fp64 statement (tests/wobj_ref.py) against closed forms, the
library's flag / workspace / refusals / schedule names, the Python argument checks, the warm-up function and the CLI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import wobj_ref as WR
import ymarg_ref as YR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def r256(n):
    return (n + 255) // 256 * 256


SMALL = ["vae", "vae_gmp", "gumbel", "marginal", "marginal-K80", "gumbel-K80"]


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("name", SMALL)
def test_unit_weights_are_the_existing_objectives(name):
    """beta = (1, 1, 0): tests/ymarg_ref.py with y summed out, the oracle's ELBO otherwise -- loss, terms and every gradient."""
    model, marginal, d, p, flat, x, eps, u = WR.setup(name)
    Cw, gw = WR.loss_and_grads(model, d, p, x, eps, u, (1.0, 1.0, 0.0), marginal)
    if marginal:
        Cr, gr = YR.loss_and_grads(d, p, x, eps)
    else:
        Cr, gr = O.loss_and_grads(model, d, p, x, eps, u, np.float64)
    for k in ("loss", "nll", "kl", "nent"):
        assert abs(Cw[k] - Cr[k]) <= 1e-12 * max(abs(Cr[k]), 1.0), k
    for k in gr:
        assert np.abs(gw[k] - gr[k]).max() <= 1e-12 * max(np.abs(gr[k]).max(), 1.0), k


@pytest.mark.parametrize("name", ["vae_gmp", "gumbel", "marginal"])
def test_zero_kl_weight_removes_every_kl_gradient_of_the_prior(name):
    """The prior's parameters enter the loss through the KL term alone: beta_z = 0 leaves them no gradient (and the loss is
    nll + beta_y ne')."""
    model, marginal, d, p, flat, x, eps, u = WR.setup(name)
    C, g = WR.loss_and_grads(model, d, p, x, eps, u, (0.0, 2.0, 0.0), marginal)
    prior = [k for k in g if k.startswith("prior_gmm") or k in ("loc", "raw_scale_diag", "mixture_logits")]
    assert prior
    for k in prior:
        assert np.abs(g[k]).max() == 0.0, k
    assert any(np.abs(g[k]).max() > 0 for k in g if k.startswith("decoder"))
    by = 2.0 if model == O.MODEL_GMVAE else 0.0
    assert abs(C["loss"] - (C["nll"] + by * C["nent"])) <= 1e-12 * abs(C["loss"])


@pytest.mark.parametrize("name", ["gumbel", "marginal"])
def test_floor_above_every_example_zeroes_the_y_term_gradient(name):
    """lambda above every example's KL_y: the y term is a constant, so the gradients are those at beta_y = 0 -- all of them."""
    model, marginal, d, p, flat, x, eps, u = WR.setup(name)
    C0, _ = WR.loss_and_grads(model, d, p, x, eps, u, (1.0, 1.0, 0.0), marginal)
    lam = C0["kl_y"].max() + 0.5
    Cf, gf = WR.loss_and_grads(model, d, p, x, eps, u, (0.25, 2.0, lam), marginal)
    Cn, gn = WR.loss_and_grads(model, d, p, x, eps, u, (0.25, 0.0, 0.0), marginal)
    assert Cf["floor"].all()
    for k in gn:
        assert np.abs(gf[k] - gn[k]).max() <= 1e-14 * max(np.abs(gn[k]).max(), 1.0), k
    assert abs(Cf["loss"] - (Cn["loss"] + 2.0 * (lam - np.log(d.K)))) <= 1e-12 * abs(Cf["loss"])
    # and with the floor off the y term does reach encoder_y
    _, g1 = WR.loss_and_grads(model, d, p, x, eps, u, (0.25, 2.0, 0.0), marginal)
    assert np.abs(g1["encoder_y_fcnet/linear_0/w"] - gn["encoder_y_fcnet/linear_0/w"]).max() > 1e-6


@pytest.mark.parametrize("name", [n for n, c in WR.CASES.items() if c[0] == "gmvae"])
def test_lambda_of_the_gpu_cases_splits_the_batch(name):
    """The condition tests/test_wobj.py asserts again, here on the fp64 statement alone: two neighbouring KL_y values more than
    1e-3 nat apart, examples on both sides of their midpoint."""
    model, marginal, d, p, flat, x, eps, u = WR.setup(name)
    lam = WR.case_lambda(name)
    C, _ = WR.loss_and_grads(model, d, p, x, eps, u, WR.WEIGHTS + (lam,), marginal)
    assert 0 < C["floor"].sum() < len(C["floor"])
    assert np.abs(C["kl_y"] - lam).min() > 5e-4


# ------------------------------------------------------------------------------------------------ the library
def test_flag_value_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    m = re.search(r"GMVAE_OBJ_WEIGHTS\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == L.OBJ_WEIGHTS == 64
    assert L.OBJ_WEIGHTS & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG |
                            L.OBJ_LABELS) == 0
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


def _offset(L, d, model, name):
    o = C.c_uint64()
    return L.lib.gmvae_workspace_offset(C.byref(d), model, name, C.byref(o)), o.value


WS_DIMS = [   # (model, B, D, Lz, K, hidden, other flags)
    ("gmvae", 1024, 784, 64, 10, (64,), 0), ("gmvae", 1024, 784, 64, 10, (64,), 4), ("gmvae", 5, 64, 4, 80, (16,), 4),
    ("gmvae", 8, 100, 5, 7, (24, 24), 0), ("vae", 9, 100, 5, 1, (24,), 0), ("vae_gmp", 9, 100, 5, 3, (24,), 0),
    ("vae", 1024, 784, 2, 1, (64,), 0),
]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"{c[0]}-B{c[1]}-K{c[4]}-f{c[6]}")
def test_workspace_grows_behind_everything(L, case):
    """With the bit: + 512 (32 rows of 4 floats) + r256(4 R) (rwk) + r256(4 B) (the floor flags) bytes, + r256(16 B) for the
    per-example partials where the dims had none (S = 1 without y summed out), behind every other buffer; no other offset moves.
    Without the bit: the size of this build at the other bits, and GMVAE_E_NET for the three names."""
    mname, B, D, Lz, K, hidden, fl = case
    model = L.MODEL_IDS[mname]
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=1, sched_flags=f)
    base, with_bit = L.workspace_bytes(mk(fl), model), L.workspace_bytes(mk(fl | L.OBJ_WEIGHTS), model)
    R = B * K if fl & L.OBJ_MARGINAL_Y else B
    assert with_bit - base == 512 + r256(4 * R) + r256(4 * B) + (0 if fl & L.OBJ_MARGINAL_Y else r256(16 * B))
    rc, ow = _offset(L, mk(fl | L.OBJ_WEIGHTS), model, b"obj_weights")
    assert rc == 0 and ow % 256 == 0 and ow + (with_bit - base) <= with_bit      # (the four regions end the workspace)
    rc, rwk = _offset(L, mk(fl | L.OBJ_WEIGHTS), model, b"rwk")
    assert rc == 0 and rwk == ow + 512
    rc, fo = _offset(L, mk(fl | L.OBJ_WEIGHTS), model, b"y_floor")
    assert rc == 0 and fo == rwk + r256(4 * R)
    for name in (b"obj_weights", b"rwk", b"y_floor"):
        assert _offset(L, mk(fl), model, name)[0] == -5
    for buf in (b"z", b"dqp", b"slabs", b"logw", b"logq"):
        assert _offset(L, mk(fl), model, buf) == _offset(L, mk(fl | L.OBJ_WEIGHTS), model, buf), buf


def test_refusals_by_code(L):
    """GMVAE_E_DIMS at S != 1 and together with the importance-weighted marginal objective, DReG or labels, from every entry that
    sizes or runs a step, before anything is touched (every pointer here is a host dummy); more than 32 steps in a graph and the
    pipeline graph."""
    u64 = C.c_uint64()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    W = L.OBJ_WEIGHTS
    mk = lambda S, f, K=10: L.make_dims(16, 784, 8, K, (64,), S=S, sched_flags=f)
    oks = [(mk(1, W), L.MODEL_GMVAE), (mk(1, W | L.OBJ_MARGINAL_Y), L.MODEL_GMVAE), (mk(1, W, 1), L.MODEL_VAE), (mk(1, W), L.MODEL_VAE_GMP)]
    for d, model in oks:
        assert L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
    cases = [(mk(3, W), m) for m in (L.MODEL_GMVAE, L.MODEL_VAE, L.MODEL_VAE_GMP)]
    cases += [(mk(1, W | L.OBJ_MARGINAL_Y_IW), L.MODEL_GMVAE), (mk(2, W | L.OBJ_MARGINAL_Y_IW), L.MODEL_GMVAE)]
    cases += [(mk(1, W | L.GRAD_DREG), L.MODEL_VAE), (mk(1, W | L.GRAD_DREG | L.OBJ_MARGINAL_Y), L.MODEL_GMVAE)]
    cases += [(mk(1, W | L.OBJ_LABELS | L.OBJ_MARGINAL_Y), L.MODEL_GMVAE)]
    for d, model in cases:
        r = C.byref(d)
        assert L.lib.gmvae_workspace_bytes(r, model, C.byref(u64)) == -2
        assert L.lib.gmvae_workspace_offset(r, model, b"obj_weights", C.byref(u64)) == -2
        assert L.lib.gmvae_step_schedule(r, model, C.create_string_buffer(48)) == -2
        assert L.lib.gmvae_step(r, model, p, None, None, p, p, p, 0, 0, None, None) == -2
        assert L.lib.gmvae_forward(r, model, p, None, None, p, p, None, None, None, None, p, 0, 0, None) == -2
        assert L.lib.gmvae_train_graph_create(r, model, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, C.byref(C.c_void_p())) == -2
        assert L.lib.gmvae_dp_step(r, model, p, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None) == -2
        assert L.lib.gmvae_dp_graph_create(r, model, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None,
                                           C.byref(C.c_void_p())) == -2
        assert L.lib.gmvae_bench_loop(r, model, p, p, p, p, p, p, p, 1, 0, C.byref(C.c_float()), None) == -2
    h = C.c_void_p()
    for d, model in oks:
        r = C.byref(d)
        assert L.lib.gmvae_train_graph_create(r, model, p, L.LABEL_SLOTS + 1, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None,
                                              C.byref(h)) == -2
        assert L.lib.gmvae_dp_graph_create(r, model, p, L.LABEL_SLOTS + 1, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None,
                                           C.byref(h)) == -2
        assert L.lib.gmvae_train_graph_create_pipeline(r, model, p, 100, p, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8,
                                                       None, C.byref(h)) == -2
    assert h.value is None


def test_bounds_and_posteriors_mask_the_bit(L):
    for fn in (L.iw_bound_enum_y_workspace_bytes, L.posterior_y_workspace_bytes, L.iw_bound_workspace_bytes):
        a = fn(L.make_dims(16, 784, 8, 10, (64,), S=5), L.MODEL_GMVAE)
        assert a == fn(L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=L.OBJ_WEIGHTS), L.MODEL_GMVAE)
    a = L.posterior_component_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5), L.MODEL_VAE_GMP)
    assert a == L.posterior_component_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=L.OBJ_WEIGHTS),
                                                      L.MODEL_VAE_GMP)


def test_schedule_names(L):
    """With the bit every step takes the general schedule -- at the sizes of the one-launch steps too."""
    gm = lambda fl, B=16: L.step_schedule(L.make_dims(B, 784, 64, 10, (64,), S=1, sched_flags=fl), L.MODEL_GMVAE)
    assert gm(0) != "general" and gm(L.OBJ_WEIGHTS) == "general+weights"
    assert gm(L.OBJ_MARGINAL_Y | L.OBJ_WEIGHTS) == "general+marginal+weights"
    assert gm(L.OBJ_WEIGHTS, 1024) == "general+weights"
    va = lambda fl: L.step_schedule(L.make_dims(1024, 784, 2, 1, (64,), S=1, sched_flags=fl), L.MODEL_VAE)
    assert va(0) != "general" and va(L.OBJ_WEIGHTS) == "general+weights"
    sk = lambda fl: L.step_schedule(L.make_dims(64, 784, 128, 10, (512,), S=1, sched_flags=fl), L.MODEL_GMVAE)
    assert sk(0) == "skinny" and sk(L.OBJ_WEIGHTS) == "general+weights"


# ------------------------------------------------------------------------------------------ the Python surface
def test_engine_and_factory_arguments(L):
    from gmvae_amd import gmvae, vae
    from gmvae_amd.engine import Engine, check_weighted_objective
    for kw in (dict(kl_weight=-1.0), dict(y_weight=-0.5), dict(y_free_nats=-1e-3), dict(kl_weight=float("nan")),
               dict(y_free_nats=float("inf"))):
        with pytest.raises(ValueError, match="finite number >= 0"):
            Engine("gmvae", 784, 8, 10, [64], weighted_objective=True, **kw)
    with pytest.raises(ValueError, match="weighted_objective=True"):
        Engine("gmvae", 784, 8, 10, [64], kl_weight=0.5)
    with pytest.raises(ValueError, match="n_samples must be 1"):
        Engine("vae", 784, 8, 1, [64], n_samples=3, weighted_objective=True)
    with pytest.raises(ValueError, match="n_samples must be 1"):
        vae.create_vae(784, 8, fcnet_hidden_sizes=[64], n_samples=3, weighted_objective=True, kl_weight=0.5)
    with pytest.raises(ValueError, match="marginal_iw"):
        gmvae.create_gmvae(784, 8, mixture_components=10, fcnet_hidden_sizes=[64], y_inference="marginal_iw", weighted_objective=True)
    with pytest.raises(ValueError, match="dreg"):
        Engine("vae", 784, 8, 1, [64], grad_estimator="dreg", weighted_objective=True)
    with pytest.raises(ValueError, match="semi_supervised"):
        Engine("gmvae", 784, 8, 10, [64], y_inference="marginal", semi_supervised=True, weighted_objective=True)
    check_weighted_objective("gmvae", "marginal", 1, "standard", False, True, 0.0, 2.0, 0.3)
    check_weighted_objective("vae", "gumbel", 5, "dreg", False, False, 1.0, 1.0, 0.0)


def test_warmup_schedule():
    from gmvae_amd import runners
    N = 8
    assert runners.kl_warmup(0, N) == 1 / 8 and runners.kl_warmup(N - 1, N) == 1.0 and runners.kl_warmup(N, N) == 1.0
    assert runners.kl_warmup(3, N) == 0.5 and runners.kl_warmup(10 ** 6, N) == 1.0
    assert runners.kl_warmup(0, 0) == 1.0 and runners.kl_warmup(5, 1) == 1.0
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    cfg = p.parse_args(["--kl_weight=0.5", "--y_weight=2", "--y_free_nats=0.3", "--kl_warmup_steps=4"])
    assert runners.objective_weights_at(cfg, 0) == (0.125, 0.5, 0.3)
    assert runners.objective_weights_at(cfg, 3) == runners.objective_weights_at(cfg, 100) == (0.5, 2.0, 0.3)


def test_runner_flags(L):
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    d = p.parse_args([])
    assert (d.kl_weight, d.y_weight, d.y_free_nats, d.kl_warmup_steps) == (1.0, 1.0, 0.0, 0)
    assert not runners.weighted_flags(run_gmvae.check_args(p, d))
    for one in (["--kl_weight=0.5"], ["--y_weight=2"], ["--y_free_nats=0.1"], ["--kl_warmup_steps=100"]):
        assert runners.weighted_flags(run_gmvae.check_args(p, p.parse_args(one)))
    run_gmvae.check_args(p, p.parse_args(["--y_inference=marginal", "--kl_weight=0.5", "--kl_warmup_steps=10"]))
    run_gmvae.check_args(p, p.parse_args(["--model=vae", "--kl_weight=4"]))
    for bad in (["--kl_weight=0.5", "--n_samples=5"], ["--kl_warmup_steps=10", "--y_inference=marginal_iw", "--n_samples=1"],
                ["--model=vae", "--y_free_nats=0.1", "--grad_estimator=dreg"],
                ["--y_inference=marginal", "--labelled_per_class=5", "--y_weight=0.5"], ["--kl_weight=-1"],
                ["--kl_warmup_steps=-3"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
