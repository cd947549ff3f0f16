"""The per-example observation mask (GMVAE_OBJ_PIXEL_MASK) without a device: the fp64 statement (tests/pmask_ref.py) against the
oracle and its own invariants, the mask recipe of the device cases, the library's flag / workspace / refusals / schedule names,
the Python argument checks and the CLI."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import pmask_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def r256(n):
    return (n + 255) // 256 * 256


_STMT = {}      # case -> (masked statement, unmasked statement, "encoder fed the unmasked x" variant): computed once, shared


def _statements(name):
    if name not in _STMT:
        model, d, p, flat, xf, eps, u, m, x = PR.setup(name)
        _STMT[name] = (PR.loss_and_grads(model, d, p, x, eps, u, m), PR.loss_and_grads(model, d, p, x, eps, u, None),
                       PR.loss_and_grads(model, d, p, x, eps, u, m, encoder_sees_mask=False))
    return _STMT[name]


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("mname", ["vae", "vae_gmp", "gmvae"])
@pytest.mark.parametrize("S", [1, 3])
def test_all_ones_mask_is_the_oracle(mname, S):
    model = O.MODEL_NAMES[mname]
    d = O.Dims(D=40, L=4, K=1 if mname == "vae" else 5, hidden=(12,), S=S, temperature=0.8)
    p = O.init_params(model, d, np.random.default_rng(2))
    x, eps, u = O.make_inputs(d, 6, model)
    Co, go = O.loss_and_grads(model, d, p, x, eps, u, np.float64)
    for mask in (None, np.ones_like(x), np.full_like(x, 255)):
        Cs, gs = PR.loss_and_grads(model, d, p, x, eps, u, mask)
        for k in ("loss", "nll", "kl", "nent"):
            assert abs(Cs[k] - Co[k]) <= 1e-12 * max(abs(Co[k]), 1.0), k
        for k in go:
            assert np.abs(gs[k] - go[k]).max() <= 1e-12 * max(np.abs(go[k]).max(), 1.0), k
        assert Cs["hid"] == 0.0 and Cs["n_missing"] == 0.0 and Cs["n_observed"] == x.size


@pytest.mark.parametrize("name", list(PR.CASES))
def test_mask_recipe_of_every_case(name):
    model, d, p, flat, xf, eps, u, m, x = PR.setup(name)
    PR.check_mask(m)
    assert m.shape == x.shape and m.dtype == np.uint8
    assert (xf[m != 0] == x[m != 0]).all() and (xf[m == 0] == 1 - x[m == 0]).all()
    if PR.CASES[name].single_pixel_row is not None:
        assert m[PR.CASES[name].single_pixel_row].sum() == 1


@pytest.mark.parametrize("name", ["vae", "vae_gmp", "gumbel", "gumbel-784", "gmvae-s3"])
def test_gates_tell_the_variants_apart(name):
    """The masked loss differs from the unmasked one and from the variant whose encoder reads the unmasked x by at least 100 x the
    1e-4 gate of the device tests."""
    (Cm, _), (Cu, _), (Cv, _) = _statements(name)
    assert abs(Cm["loss"] - Cu["loss"]) >= 100 * 1e-4 * abs(Cm["loss"]), (Cm["loss"], Cu["loss"])
    assert abs(Cm["loss"] - Cv["loss"]) >= 100 * 1e-4 * abs(Cm["loss"]), (Cm["loss"], Cv["loss"])


@pytest.mark.parametrize("name", ["vae", "vae_gmp", "gumbel", "gmvae-s3", "gumbel-d99"])
def test_flip_invariance_and_dead_columns(name):
    """The statement does not see x at a missing pixel -- exactly --, and the dead columns (missing in every row) leave exact
    zeros: their rows of every encoder first-layer weight gradient, their columns of the decoder's output weight and bias
    gradients."""
    model, d, p, flat, xf, eps, u, m, x = PR.setup(name)
    (Cm, gm), _, _ = _statements(name)
    Cf, gf = PR.loss_and_grads(model, d, p, xf, eps, u, m)
    for k in ("loss", "nll", "kl", "nent"):
        assert Cf[k] == Cm[k], k
    for k in gm:
        assert np.array_equal(gf[k], gm[k]), k
    assert Cf["hid"] != Cm["hid"]                     # (the held-out score is the one reader of x there)
    dead = list(PR.dead_columns(d.D))
    nl = len(d.hidden)
    for net in ("encoder_y", "encoder_gmm", "encoder"):
        k = f"{net}_fcnet/linear_0/w"
        if k in gm:
            assert (gm[k][dead, :] == 0).all(), k
            assert np.abs(gm[k][:d.D]).max() > 0
    assert (gm[f"decoder_fcnet/linear_{nl}/w"][:, dead] == 0).all() and (gm[f"decoder_fcnet/linear_{nl}/b"][dead] == 0).all()
    assert Cm["n_missing"] + Cm["n_observed"] == x.size and Cm["n_observed"] == (m != 0).sum()


# ------------------------------------------------------------------------------------------------ the library
def test_flag_value_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    m = re.search(r"GMVAE_OBJ_PIXEL_MASK\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == L.OBJ_PIXEL_MASK == 512
    assert L.OBJ_PIXEL_MASK & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG |
                               L.OBJ_LABELS | L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH) == 0
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


def test_schedule_names(L):
    """With the bit every step takes the general schedule: at the one-launch sizes, the skinny sizes and the config-5 sizes (no
    "+planes")."""
    M = L.OBJ_PIXEL_MASK
    gm = lambda fl, B=1024: L.step_schedule(L.make_dims(B, 784, 64, 10, (64,), sched_flags=fl), L.MODEL_GMVAE)
    assert gm(0) != "general" and gm(M) == "general+mask" and gm(M, 16) == "general+mask"
    sk = lambda fl: L.step_schedule(L.make_dims(64, 784, 128, 10, (512,), sched_flags=fl), L.MODEL_GMVAE)
    assert sk(0) == "skinny" and sk(M) == "general+mask"
    c5 = lambda fl: L.step_schedule(L.make_dims(25600, 3072, 128, 64, (512, 512), sched_flags=fl), L.MODEL_GMVAE)
    assert c5(0) == "general+planes" and c5(M) == "general+mask"
    va = lambda fl: L.step_schedule(L.make_dims(1024, 784, 2, 1, (64,), sched_flags=fl), L.MODEL_VAE)
    assert va(0) != "general" and va(M) == "general+mask"
    assert L.step_schedule(L.make_dims(8, 96, 4, 6, (16,), S=3, sched_flags=M), L.MODEL_GMVAE) == "general+mask"


def _offset(L, d, model, name):
    o = C.c_uint64()
    return L.lib.gmvae_workspace_offset(C.byref(d), model, name, C.byref(o)), o.value


WS_DIMS = [   # (model, B, D, Lz, K, hidden, S)
    ("gmvae", 1024, 784, 64, 10, (64,), 1), ("gmvae", 5, 99, 5, 7, (24,), 1), ("gmvae", 4, 96, 4, 6, (16,), 3),
    ("vae", 9, 100, 5, 1, (24,), 1), ("vae_gmp", 9, 100, 5, 3, (24,), 1), ("vae", 1024, 784, 2, 1, (64,), 1), ("vae", 3, 1, 2, 1, (4,), 2),
]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"{c[0]}-B{c[1]}-D{c[2]}-S{c[6]}")
def test_workspace_grows_behind_everything(L, case):
    """With the bit: + 32 r256(B D) (the masks) + r256(B D) (x~) + r256(4 R ceil(D / 32)) (the held-out partials) + r256(8 B) (the
    counts) bytes behind every other buffer; no other offset moves.  Without it: GMVAE_E_NET for the name."""
    mname, B, D, Lz, K, hidden, S = case
    model = L.MODEL_IDS[mname]
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=f)
    base, with_bit = L.workspace_bytes(mk(0), model), L.workspace_bytes(mk(L.OBJ_PIXEL_MASK), model)
    grow = L.LABEL_SLOTS * r256(B * D) + r256(B * D) + r256(4 * B * S * ((D + 31) // 32)) + r256(8 * B)
    assert with_bit - base == grow
    rc, off = _offset(L, mk(L.OBJ_PIXEL_MASK), model, b"pixel_mask")
    assert rc == 0 and off % 256 == 0 and off + grow <= with_bit
    assert _offset(L, mk(0), model, b"pixel_mask")[0] == -5
    for buf in (b"z", b"dqp", b"slabs", b"logw", b"logq", b"g", b"eps"):
        a = _offset(L, mk(0), model, buf)
        assert a == _offset(L, mk(L.OBJ_PIXEL_MASK), model, buf) and a[0] == 0 and a[1] < off, buf


def test_refusals_by_code(L):
    """GMVAE_E_DIMS together with every other objective / estimator bit, from every entry that sizes or runs a step, before
    anything is touched (every pointer here is a host dummy); more than 32 steps in a graph, the pipeline graph, and the three
    evaluators that would score the unobserved pixels."""
    u64 = C.c_uint64()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    M = L.OBJ_PIXEL_MASK
    mk = lambda S, f, K=10: L.make_dims(16, 784, 8, K, (64,), S=S, sched_flags=f)
    oks = [(mk(1, M), L.MODEL_GMVAE), (mk(3, M), L.MODEL_GMVAE), (mk(1, M, 1), L.MODEL_VAE), (mk(2, M), L.MODEL_VAE_GMP)]
    for d, model in oks:
        assert L.lib.gmvae_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
        assert L.lib.gmvae_iw_bound_workspace_bytes(C.byref(d), model, C.byref(u64)) == 0
    G = L.MODEL_GMVAE
    cases = [(mk(1, M | L.OBJ_MARGINAL_Y), G), (mk(2, M | L.OBJ_MARGINAL_Y_IW), G), (mk(2, M | L.GRAD_DREG, 1), L.MODEL_VAE),
             (mk(1, M | L.GRAD_DREG | L.OBJ_MARGINAL_Y), G), (mk(1, M | L.OBJ_LABELS | L.OBJ_MARGINAL_Y), G),
             (mk(1, M | L.OBJ_WEIGHTS), G), (mk(1, M | L.OBJ_WEIGHTS, 1), L.MODEL_VAE), (mk(1, M | L.Y_TEMP_DEV), G),
             (mk(3, M | L.Y_STRAIGHT_THROUGH), G)]
    for d, model in cases:
        r = C.byref(d)
        assert L.lib.gmvae_workspace_bytes(r, model, C.byref(u64)) == -2
        assert L.lib.gmvae_workspace_offset(r, model, b"pixel_mask", C.byref(u64)) == -2
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
    # the evaluators that would score the unobserved pixels
    d = mk(2, M)
    r = C.byref(d)
    assert L.lib.gmvae_iw_bound_enum_y_workspace_bytes(r, G, C.byref(u64)) == -2
    assert L.lib.gmvae_posterior_y_workspace_bytes(r, G, C.byref(u64)) == -2
    assert L.lib.gmvae_posterior_component_workspace_bytes(r, L.MODEL_VAE_GMP, C.byref(u64)) == -2
    assert L.lib.gmvae_iw_bound_enum_y(r, G, p, p, 4, None, None, p, p, 0, 0, None) == -2
    assert L.lib.gmvae_posterior_y(r, G, p, p, 4, None, None, None, p, p, 0, 0, None) == -2
    assert L.lib.gmvae_posterior_component(r, L.MODEL_VAE_GMP, p, p, 4, None, None, None, p, p, 0, 0, None) == -2


def test_iw_bound_workspace_holds_the_masks(L):
    """gmvae_iw_bound honours the bit: its workspace opens with the forward's, masks included."""
    mk = lambda f: L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=f)
    a, b = L.iw_bound_workspace_bytes(mk(0), L.MODEL_GMVAE), L.iw_bound_workspace_bytes(mk(L.OBJ_PIXEL_MASK), L.MODEL_GMVAE)
    assert b - a == L.workspace_bytes(mk(L.OBJ_PIXEL_MASK), L.MODEL_GMVAE) - L.workspace_bytes(mk(0), L.MODEL_GMVAE)


# ------------------------------------------------------------------------------------------ the Python surface
def test_check_pixel_mask(L):
    from gmvae_amd.engine import check_pixel_mask
    check_pixel_mask("gmvae", "gumbel", "standard", False, False, False, "relaxed", True)
    check_pixel_mask("vae", "gumbel", "standard", False, False, False, "relaxed", True)
    check_pixel_mask("gmvae", "marginal_iw", "dreg", True, True, True, "straight_through", False)      # off: nothing to refuse
    bad = [(("gmvae", "marginal", "standard", False, False, False, "relaxed"), "y_inference"),
           (("gmvae", "marginal_iw", "standard", False, False, False, "relaxed"), "y_inference"),
           (("vae", "gumbel", "dreg", False, False, False, "relaxed"), "dreg"),
           (("gmvae", "gumbel", "standard", True, False, False, "relaxed"), "semi_supervised"),
           (("gmvae", "gumbel", "standard", False, True, False, "relaxed"), "weighted_objective"),
           (("gmvae", "gumbel", "standard", False, False, True, "relaxed"), "temperature_on_device"),
           (("gmvae", "gumbel", "standard", False, False, False, "straight_through"), "y_estimator")]
    for args, what in bad:
        with pytest.raises(ValueError, match=what):
            check_pixel_mask(*args, True)


def test_runner_flags(L):
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    d = p.parse_args([])
    assert d.missing_rate == 0.0 and d.missing_seed == 0
    assert runners.missing_mask(run_gmvae.check_args(p, d), "train", 10, 7) is None
    ok = run_gmvae.check_args(p, p.parse_args(["--missing_rate=0.5", "--missing_seed=3", "--iw_samples=7", "--n_samples=3"]))
    run_gmvae.check_args(p, p.parse_args(["--model=vae_gmp", "--missing_rate=0.25"]))
    for bad in (["--missing_rate=0.5", "--y_inference=marginal"], ["--missing_rate=0.5", "--y_inference=marginal_iw"],
                ["--missing_rate=0.5", "--model=vae", "--grad_estimator=dreg"], ["--missing_rate=0.5", "--kl_weight=0.5"],
                ["--missing_rate=0.5", "--kl_warmup_steps=10"], ["--missing_rate=0.5", "--temperature=0.5"],
                ["--missing_rate=0.5", "--y_estimator=straight_through"], ["--missing_rate=0.5", "--iw_enum_samples=4"],
                ["--missing_rate=0.5", "--posterior_samples=4"],
                ["--missing_rate=0.5", "--model=vae_gmp", "--mode=eval", "--component_posterior_samples=4"],
                ["--missing_rate=1.0"], ["--missing_rate=-0.1"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    # one fixed mask per dataset row: a function of the seed and the split alone, at the asked rate
    a, b = runners.missing_mask(ok, "train", 400, 50), runners.missing_mask(ok, "train", 400, 50)
    assert a.dtype == np.uint8 and a.shape == (400, 50) and np.array_equal(a, b) and set(np.unique(a)) == {0, 1}
    assert abs(a.mean() - 0.5) < 0.02
    assert not np.array_equal(a, runners.missing_mask(ok, "test", 400, 50))
    other = argparse.Namespace(**{**vars(ok), "missing_seed": 4})
    assert not np.array_equal(a, runners.missing_mask(other, "train", 400, 50))
