"""CPU side of the semi-supervised GMVAE objective (include/gmvae_hip.h GMVAE_OBJ_LABELS): the flag, the workspace growth and
the two named regions, every refusal and the schedule names of the C ABI, the Engine / factory / runner arguments, the selection
rule of --labelled_per_class, and the fp64 statement itself (tests/semisup_ref.py) against tests/ymarg_iw_ref.py and its own
closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import semisup_ref as SR
import ymarg_iw_ref as YI

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
def test_flag_slots_and_abi_version(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    m = re.search(r"GMVAE_OBJ_LABELS\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == L.OBJ_LABELS == 32
    m = re.search(r"#define\s+GMVAE_LABEL_SLOTS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == L.LABEL_SLOTS == 32
    assert L.OBJ_LABELS & (L.SCHED_SAFE | L.SCHED_EVAL_IMAGES_VALID | L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG) == 0
    assert L.lib.gmvae_abi_version() == 7 == L.ABI_VERSION


def _offset(L, d, name):
    o = C.c_uint64()
    return L.lib.gmvae_workspace_offset(C.byref(d), L.MODEL_GMVAE, name, C.byref(o)), o.value


WS_DIMS = [   # (B, D, Lz, K, hidden, S, objective / estimator flags)
    (1024, 784, 64, 10, (64,), 1, 4), (1024, 784, 64, 10, (64,), 1, 8), (1024, 784, 64, 10, (64,), 5, 8),
    (6, 200, 8, 10, (64,), 3, 8), (5, 200, 8, 80, (64,), 2, 8 | 16), (9, 200, 16, 7, (64, 64), 2, 8 | 16), (7, 100, 5, 3, (24,), 1, 4 | 16),
]


@pytest.mark.parametrize("case", WS_DIMS, ids=lambda c: f"B{c[0]}-K{c[3]}-S{c[5]}-f{c[6]}")
def test_workspace_grows_behind_everything(L, case):
    """With the bit: + r256(4 * 32 * B4) + 256 + r256(12 * B) bytes (labels, sup_weight, the per-example triples), behind every
    other buffer (DReG's v included), both named offsets 16-byte aligned, every label slot too; no other offset moves.  Without
    the bit: the size of this build at the other bits, and GMVAE_E_NET for the two names."""
    B, D, Lz, K, hidden, S, fl = case
    mk = lambda f: L.make_dims(B, D, Lz, K, hidden, S=S, sched_flags=f)
    base, with_bit = L.workspace_bytes(mk(fl), L.MODEL_GMVAE), L.workspace_bytes(mk(fl | L.OBJ_LABELS), L.MODEL_GMVAE)
    B4 = (B + 3) // 4 * 4
    assert with_bit - base == r256(4 * L.LABEL_SLOTS * B4) + 256 + r256(12 * B)
    rc, lab = _offset(L, mk(fl | L.OBJ_LABELS), b"labels")
    assert rc == 0 and lab % 16 == 0 and (4 * B4) % 16 == 0 and lab == base
    rc, sw = _offset(L, mk(fl | L.OBJ_LABELS), b"sup_weight")
    assert rc == 0 and sw % 16 == 0 and sw == lab + r256(4 * L.LABEL_SLOTS * B4)
    rc, vs = _offset(L, mk(fl | L.OBJ_LABELS), b"vs")
    if fl & L.GRAD_DREG and fl & L.OBJ_MARGINAL_Y_IW and S > 1:
        assert rc == 0 and vs + r256(4 * B * S * K) == lab
    else:
        assert rc == -5
    for name in (b"labels", b"sup_weight"):
        assert _offset(L, mk(fl), name)[0] == -5
    for buf in (b"z", b"dqp", b"slabs", b"logw", b"dlogits", b"logits"):
        assert _offset(L, mk(fl), buf) == _offset(L, mk(fl | L.OBJ_LABELS), buf), buf


def test_refusals_by_code(L):
    """GMVAE_E_MODEL for the VAE family, GMVAE_E_DIMS for the Gumbel GMVAE, from every entry that sizes or runs a step, before
    anything is touched (every pointer here is a host dummy); more than 32 steps in a graph and the pipeline graph."""
    u64 = C.c_uint64()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    ok = L.make_dims(16, 784, 8, 10, (64,), S=2, sched_flags=L.OBJ_LABELS | L.OBJ_MARGINAL_Y_IW)
    assert L.lib.gmvae_workspace_bytes(C.byref(ok), L.MODEL_GMVAE, C.byref(u64)) == 0
    cases = [(L.make_dims(16, 784, 8, 10, (64,), S=S, sched_flags=L.OBJ_LABELS), L.MODEL_GMVAE, -2) for S in (1, 3)]
    cases += [(L.make_dims(16, 784, 8, 10, (64,), S=1, sched_flags=L.OBJ_LABELS | L.GRAD_DREG), L.MODEL_GMVAE, -2)]
    cases += [(L.make_dims(16, 784, 8, 10, (64,), S=2, sched_flags=L.OBJ_LABELS), m, -3) for m in (L.MODEL_VAE, L.MODEL_VAE_GMP)]
    cases += [(L.make_dims(16, 784, 8, 10, (64,), S=1, sched_flags=L.OBJ_LABELS | L.OBJ_MARGINAL_Y), L.MODEL_VAE, -3)]
    for d, model, code in cases:
        r = C.byref(d)
        assert L.lib.gmvae_workspace_bytes(r, model, C.byref(u64)) == code
        assert L.lib.gmvae_workspace_offset(r, model, b"labels", C.byref(u64)) == code
        assert L.lib.gmvae_step_schedule(r, model, C.create_string_buffer(48)) == code
        assert L.lib.gmvae_step(r, model, p, None, None, p, p, p, 0, 0, None, None) == code
        assert L.lib.gmvae_forward(r, model, p, None, None, p, p, None, None, None, None, p, 0, 0, None) == code
        assert L.lib.gmvae_train_graph_create(r, model, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, C.byref(C.c_void_p())) == code
        assert L.lib.gmvae_dp_step(r, model, p, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None) == code
        assert L.lib.gmvae_dp_graph_create(r, model, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None,
                                           C.byref(C.c_void_p())) == code
        assert L.lib.gmvae_bench_loop(r, model, p, p, p, p, p, p, p, 1, 0, C.byref(C.c_float()), None) == code
    # one label set per step of a graph: 33 steps are refused, with and without a communicator; so is the pipeline graph
    r = C.byref(ok)
    h = C.c_void_p()
    assert L.lib.gmvae_train_graph_create(r, L.MODEL_GMVAE, p, L.LABEL_SLOTS + 1, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None,
                                          C.byref(h)) == -2
    assert L.lib.gmvae_dp_graph_create(r, L.MODEL_GMVAE, p, L.LABEL_SLOTS + 1, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None,
                                       C.byref(h)) == -2
    assert L.lib.gmvae_train_graph_create_pipeline(r, L.MODEL_GMVAE, p, 100, p, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8,
                                                   None, C.byref(h)) == -2
    assert h.value is None


def test_bounds_and_posteriors_mask_the_bit(L):
    for fn in (L.iw_bound_enum_y_workspace_bytes, L.posterior_y_workspace_bytes):
        a = fn(L.make_dims(16, 784, 8, 10, (64,), S=5), L.MODEL_GMVAE)
        for fl in (L.OBJ_LABELS, L.OBJ_LABELS | L.OBJ_MARGINAL_Y_IW, L.OBJ_LABELS | L.OBJ_MARGINAL_Y_IW | L.GRAD_DREG):
            assert a == fn(L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=fl), L.MODEL_GMVAE)
    a = L.posterior_component_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5), L.MODEL_VAE_GMP)
    assert a == L.posterior_component_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=L.OBJ_LABELS),
                                                      L.MODEL_VAE_GMP)
    a = L.iw_bound_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5), L.MODEL_GMVAE)
    assert a == L.iw_bound_workspace_bytes(L.make_dims(16, 784, 8, 10, (64,), S=5, sched_flags=L.OBJ_LABELS), L.MODEL_GMVAE)


def test_schedule_names(L):
    cfg2 = dict(B=1024, D=784, L=64, K=10, hidden=(64,))
    name = lambda S, fl: L.step_schedule(L.make_dims(S=S, sched_flags=fl, **cfg2), L.MODEL_GMVAE)
    assert name(5, L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS) == "general+marginal_iw+labels"
    assert name(1, L.OBJ_MARGINAL_Y | L.OBJ_LABELS) == "general+marginal+labels"
    assert name(1, L.OBJ_MARGINAL_Y | L.OBJ_LABELS | L.GRAD_DREG) == "general+marginal+labels+dreg"
    assert name(5, L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS | L.GRAD_DREG) == "general+marginal_iw+labels+dreg"
    assert name(5, L.OBJ_MARGINAL_Y_IW) == "general+marginal_iw" and name(1, L.OBJ_MARGINAL_Y | L.GRAD_DREG) == "general+marginal+dreg"


# ------------------------------------------------------------------------------------------ the Python surface
def test_engine_and_factory_arguments(L):
    from gmvae_amd import gmvae
    from gmvae_amd.engine import Engine
    with pytest.raises(ValueError, match="GMVAE"):
        Engine("vae", 784, 8, 1, [64], semi_supervised=True)
    with pytest.raises(ValueError, match="GMVAE"):
        Engine("vae_gmp", 784, 8, 10, [64], semi_supervised=True)
    for kw in (dict(), dict(n_samples=3), dict(y_inference="gumbel")):
        with pytest.raises(ValueError, match="marginal.*marginal_iw"):
            Engine("gmvae", 784, 8, 10, [64], semi_supervised=True, **kw)
        with pytest.raises(ValueError, match="marginal.*marginal_iw"):
            gmvae.create_gmvae(784, 8, mixture_components=10, fcnet_hidden_sizes=[64], semi_supervised=True, **kw)
    with pytest.raises(ValueError, match="sup_weight"):
        Engine("gmvae", 784, 8, 10, [64], y_inference="marginal", semi_supervised=True, sup_weight=-1.0)


def test_runner_flags(L):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    d = p.parse_args([])
    assert d.labelled_per_class == 0 and d.sup_weight == 1.0
    c = run_gmvae.check_args(p, p.parse_args(["--y_inference=marginal", "--labelled_per_class", "20", "--sup_weight", "0.5"]))
    assert (c.labelled_per_class, c.sup_weight) == (20, 0.5)
    run_gmvae.check_args(p, p.parse_args(["--y_inference=marginal_iw", "--n_samples=3", "--labelled_per_class=5"]))
    for bad in (["--labelled_per_class=5"], ["--labelled_per_class=5", "--model=vae"], ["--y_inference=marginal", "--labelled_per_class=-1"],
                ["--y_inference=marginal", "--labelled_per_class=5", "--sup_weight=-2"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))


def test_selection_rule_of_labelled_per_class():
    """N rows per class, the first N of the class in one seeded permutation of the whole split; the same rows whatever the
    number of ranks (the shards of world 2 are slices of world 1's choice); deterministic in the seed."""
    from gmvae_amd import parallel, runners
    lab = np.random.default_rng(3).integers(0, 10, 8192)
    y = runners.select_labelled(lab, 20, 5)
    assert y.dtype == np.int32 and y.shape == lab.shape
    on = y >= 0
    assert np.array_equal(y[on], lab[on]) and (y[~on] == -1).all()
    assert np.array_equal(np.bincount(y[on], minlength=10), np.full(10, 20))
    assert np.array_equal(y, runners.select_labelled(lab, 20, 5))
    assert not np.array_equal(y, runners.select_labelled(lab, 20, 6))
    perm = np.random.default_rng(5).permutation(lab.size)
    for c in range(10):
        assert set(np.flatnonzero(y == c)) == set(perm[lab[perm] == c][:20])
    assert (runners.select_labelled(lab, 0, 5) == -1).all()
    few = runners.select_labelled(np.array([0, 1, 1, 2, 2, 2]), 2, 0)                 # a class with fewer rows shows them all
    assert np.array_equal(np.bincount(few[few >= 0], minlength=3), [1, 2, 2])
    # create_device_dataset cuts each rank's shard out of the whole split's choice
    shards = [parallel.shard_rows(lab.size, r, 2) for r in range(2)]
    assert np.array_equal(np.concatenate([y[a:b] for a, b in shards]), y)
    src = open(os.path.join(ROOT, "gmvae_amd", "runners.py")).read()
    assert "select_labelled(lab, lpc, config.random_seed or 0)[a:b]" in src


# ---------------------------------------------------------------------------------------- the fp64 statement
def _setup(d, B, S, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.1, p[k].shape)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * S * d.K, d.L))
    return p, x, eps


CASES = [(O.Dims(D=30, L=3, K=4, hidden=(12, 9)), 5, 1), (O.Dims(D=30, L=3, K=4, hidden=(12,), sigma_min=0.9), 3, 4),
         (O.Dims(D=30, L=3, K=5, hidden=(12,), act="tanh"), 6, 2)]


@pytest.mark.parametrize("d,B,S", CASES, ids=[f"K{c[0].K}-S{c[2]}" for c in CASES])
def test_unlabelled_statement_is_the_marginal_iw_statement(d, B, S):
    p, x, eps = _setup(d, B, S, seed=S)
    Cr, gr = YI.loss_and_grads(d, p, x, eps, S)
    for yo in (np.full(B, -1), np.full(B, d.K), np.array([-1, d.K, -7, 99, d.K + 1, -1])[:B]):      # out of range is unlabelled
        for alpha in (0.0, 0.7):
            Cs, gs = SR.loss_and_grads(d, p, x, eps, S, yo, alpha)
            for k in ("loss", "nll", "kl", "nent"):
                assert abs(Cs[k] - Cr[k]) <= 1e-12 * max(1.0, abs(Cr[k])), k
            np.testing.assert_allclose(Cs["dlogits"], Cr["dlogits"], rtol=1e-12, atol=1e-15)
            assert (Cs["ce"], Cs["n_labelled"], Cs["hits"]) == (0.0, 0, 0)
            for k, ref in gr.items():
                assert np.abs(gs[k] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0), k


@pytest.mark.parametrize("d,B,S", CASES, ids=[f"K{c[0].K}-S{c[2]}" for c in CASES])
def test_labelled_statement_closed_forms(d, B, S):
    """All labelled: L_b = l_bc + alpha ce_b, dlogits = alpha (q - onehot) / B, no entropy; mixed: the tail identity
    [0] = [1] + [2] + [3] + alpha [5] at S = 1 (an inequality at S > 1, as for the marginal_iw objective) and the counts."""
    p, x, eps = _setup(d, B, S, seed=10 + S)
    alpha = 0.7
    K = d.K
    c = np.random.default_rng(S).integers(0, K, B)
    Cs, gs = SR.loss_and_grads(d, p, x, eps, S, c, alpha)
    q, ell = Cs["q"], Cs["ell"]
    lnq = np.log(q)
    onehot = np.eye(K)[c]
    ce = -(onehot * lnq).sum(axis=1)
    np.testing.assert_allclose(Cs["per_example"], (onehot * ell).sum(axis=1) + alpha * ce, rtol=1e-12)
    np.testing.assert_allclose(Cs["dlogits"], alpha * (q - onehot) / B, rtol=1e-10, atol=1e-15)
    assert Cs["nent"] == 0.0 and Cs["n_labelled"] == B and abs(Cs["ce"] - ce.sum()) <= 1e-12 * ce.sum()
    assert Cs["hits"] == int((q.argmax(axis=1) == c).sum())
    lw = Cs["rows"][:, 3].reshape(B, S, K)
    ell_ref = -(np.log(np.exp(lw - lw.max(axis=1, keepdims=True)).sum(axis=1)) + lw.max(axis=1) - np.log(S))
    np.testing.assert_allclose(ell, ell_ref, rtol=1e-12)
    # alpha = 0: encoder_y sees nothing of an all-labelled batch
    _, g0 = SR.loss_and_grads(d, p, x, eps, S, c, 0.0)
    for k, v in g0.items():
        if k.startswith("encoder_y_fcnet/"):
            assert not v.any(), k
    # mixed batch: the tail identity and the per-example split
    mixed = c.copy()
    mixed[::2] = -1
    Cm, _ = SR.loss_and_grads(d, p, x, eps, S, mixed, alpha)
    Cu, _ = YI.loss_and_grads(d, p, x, eps, S)
    parts = Cm["nll"] + Cm["kl"] + Cm["nent"] + alpha * Cm["ce"] / B
    if S == 1:
        assert abs(Cm["loss"] - parts) <= 1e-12 * abs(Cm["loss"])
    else:                                  # (-log mean_s w <= mean_s -log w: the importance-weighted term is below the terms' mean)
        assert Cm["loss"] < parts
    np.testing.assert_allclose(Cm["per_example"][::2], Cu["per_example"][::2], rtol=1e-12)
    np.testing.assert_allclose(Cm["per_example"][1::2], Cs["per_example"][1::2], rtol=1e-12)
    assert Cm["n_labelled"] == len(mixed[1::2])


def test_dreg_statement_with_labels_moves_only_the_inference_network():
    d, B, S = CASES[1]
    p, x, eps = _setup(d, B, S, seed=4)
    c = np.array([1, -1, 3])
    Cs, gs = SR.loss_and_grads(d, p, x, eps, S, c, 0.7)
    Cd, gd = SR.loss_and_grads(d, p, x, eps, S, c, 0.7, estimator="dreg")
    assert Cs["loss"] == Cd["loss"]
    moved = 0.0
    for k, ref in gs.items():
        if k.startswith("encoder_gmm_fcnet/"):
            moved = max(moved, np.abs(gd[k] - ref).max() / max(np.abs(ref).max(), 1e-30))
        else:
            assert np.array_equal(gd[k], ref), k
    assert moved > 1e-3
    # the row weights: [k == c] softmax_s for the labelled examples, q softmax_s for the other
    w, v = Cs["w"].reshape(B, S, d.K), Cs["v"].reshape(B, S, d.K)
    np.testing.assert_allclose(v.sum(axis=1), 1.0, rtol=1e-12)
    for b, cb in enumerate(c):
        wk = np.eye(d.K)[cb] if cb >= 0 else Cs["q"][b]
        np.testing.assert_allclose(w[b], wk[None, :] * v[b], rtol=1e-12)
