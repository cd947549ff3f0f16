"""Gradient clipping by the global norm (GMVAE_OPT_CLIP_NORM) without a device: the statement itself, the flag, the workspace
regions, the schedule names, the constructors' refusals and the argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import clip_ref
from test_step_inputs_cpu import CONSTRUCTIONS

E_NET = -5
E_DIMS = -2


def r256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def _buf(g, count=1.0, loss=3.0):
    b = np.zeros(len(g) + clip_ref.TAIL, dtype=np.float32)
    b[:len(g)] = g
    b[len(g)], b[len(g) + 4] = loss, count
    return b


# ------------------------------------------------------------------ the statement
@pytest.mark.parametrize("count", [1.0, 100.0, 1024.0])
@pytest.mark.parametrize("ratio", [0.01, 0.5, 0.998, 1.002, 10.0, math.inf])
def test_statement_clips_to_the_threshold_and_keeps_the_direction(count, ratio):
    rng = np.random.default_rng(7)
    g = rng.standard_normal(1028).astype(np.float32) * count
    b = _buf(g, count)
    norm = np.linalg.norm(g.astype(np.float64)) / count
    Cthr = float(np.float32(ratio * norm))
    n, d, clipped, skip = clip_ref.record(b, Cthr)
    assert not skip and abs(n - norm) <= 1e-12 * norm
    out = clip_ref.clipped_mean_gradient(b, Cthr)
    assert abs(np.linalg.norm(out) - min(norm, Cthr)) <= 1e-12 * norm
    mean = g.astype(np.float64) / count
    cos = float(out @ mean) / (np.linalg.norm(out) * np.linalg.norm(mean))
    assert abs(cos - 1.0) <= 1e-12
    assert clipped == (norm > Cthr)
    if not clipped:
        assert d == count and np.array_equal(out, mean)


def test_statement_special_cases():
    ones = np.ones(16, dtype=np.float32)
    # SS = 0: d = count, nothing divided by zero
    n, d, clipped, skip = clip_ref.record(_buf(np.zeros(16), 5.0), 1.0)
    assert (n, d, clipped, skip) == (0.0, 5.0, False, False)
    # C = inf: reports, never clips
    n, d, clipped, skip = clip_ref.record(_buf(1e6 * ones, 2.0), math.inf)
    assert n == 2e6 and d == 2.0 and not clipped and not skip
    # C <= 0 or NaN: skipped
    for bad in (0.0, -1.0, math.nan):
        assert clip_ref.record(_buf(ones), bad)[3]
        assert clip_ref.clipped_mean_gradient(_buf(ones), bad) is None
    # a NaN or inf element, a non-finite loss sum: skipped
    for v in (math.nan, math.inf, -math.inf):
        g = ones.copy()
        g[3] = v
        assert clip_ref.record(_buf(g), 1.0)[3]
        assert clip_ref.record(_buf(ones, loss=v), 1.0)[3]
    # magnitudes whose squares leave fp32
    big = ones.copy()
    big[0] = 3e19
    n, d, clipped, skip = clip_ref.record(_buf(big), 1.0)
    assert not skip and math.isfinite(n) and abs(n - 3e19) < 1e-6 * 3e19 and clipped
    n, d, clipped, skip = clip_ref.record(_buf(np.full(16, 1e-25, dtype=np.float32)), 1.0)
    assert not skip and abs(n - 4 * float(np.float32(1e-25))) <= 1e-12 * n and n > 0


def test_check_record_holds_the_bounds():
    b = _buf(np.arange(1, 9, dtype=np.float32), 4.0)
    n, d, clipped, skip = clip_ref.record(b, 1.0)
    good = np.array([n, d, 1.0, 3.0], dtype=np.float32)
    assert clip_ref.check_record(good, b, 1.0) <= 0.5 + 1e-9          # (one rounding: half of the 2 u bound)
    for bad in (good * np.float32([1 + 4 * clip_ref.U, 1, 1, 1]), good * np.float32([1, 1 - 4 * clip_ref.U, 1, 1]),
                np.float32([n, d, 0.0, 3.0]), np.float32([n, d, 1.0, 2.0])):
        with pytest.raises(AssertionError):
            clip_ref.check_record(bad, b, 1.0)
    with pytest.raises(AssertionError):
        clip_ref.check_record(good, b, 0.0)                           # (a skip needs a NaN guard)
    assert clip_ref.flag_band(_buf(np.float32([3.0, 4.0]), 5.0), 1.0) and not clip_ref.flag_band(b, 1.0)


# ------------------------------------------------------------------ the ABI
def test_flag_abi_and_exports(L):
    assert L.OPT_CLIP_NORM == 1024
    others = [L.SCHED_SAFE, L.SCHED_EVAL_IMAGES_VALID, L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.GRAD_DREG, L.OBJ_LABELS,
              L.OBJ_WEIGHTS, L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH, L.OBJ_PIXEL_MASK]
    assert all(L.OPT_CLIP_NORM & o == 0 for o in others) and len(set(others)) == len(others)
    assert L.ABI_VERSION == 7 and L.lib.gmvae_abi_version() == 7
    assert "gmvae_grad_clip" in L.EXPORTS and "gmvae_grad_clip_scratch_bytes" in L.EXPORTS
    from gmvae_amd.engine import STEP_INPUTS
    assert len(STEP_INPUTS) == 4 and all(inp.bit != L.OPT_CLIP_NORM for inp in STEP_INPUTS)


def test_entry_point_argument_checks(L):
    """The two entry points refuse before any launch (every pointer is a host dummy)."""
    b = C.c_uint64()
    q = L.lib.gmvae_grad_clip_scratch_bytes
    assert q(0, C.byref(b)) == E_DIMS and q(6, C.byref(b)) == E_DIMS and q(4, None) == -1
    for P, want in ((4, 256), (1024, 256), (1028, 256), (32 * 1024, 256), (32 * 1024 + 4, 512), (2 ** 20 + 4, r256(8 * 1025))):
        assert q(P, C.byref(b)) == 0 and b.value == want, P
    buf = C.create_string_buffer(4096 + 16)
    base = (C.addressof(buf) + 15) // 16 * 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    f = L.lib.gmvae_grad_clip
    assert f(None, 4, p, p, p, None) == -1 and f(p, 4, None, p, p, None) == -1
    assert f(p, 4, p, None, p, None) == -1 and f(p, 4, p, p, None, None) == -1
    assert f(p, 0, p, p, p, None) == E_DIMS and f(p, 6, p, p, p, None) == E_DIMS
    assert f(odd, 4, p, p, p, None) == -4 and f(p, 4, p, p, odd, None) == -4


def _flags_of(L, y_inference, ge, want):
    from gmvae_amd.engine import STEP_INPUTS
    flags = {"gumbel": 0, "marginal": L.OBJ_MARGINAL_Y, "marginal_iw": L.OBJ_MARGINAL_Y_IW}[y_inference]
    flags |= L.GRAD_DREG if ge == "dreg" else 0
    for inp in STEP_INPUTS:
        flags |= inp.bit if inp.option in want else 0
    return flags


@pytest.mark.parametrize("hidden", [(64,), (512,), (24, 24)])
@pytest.mark.parametrize("B", [1, 16, 1024])
def test_workspace_grows_by_the_three_regions(L, B, hidden):
    """bytes(with the bit) - bytes(without) = 256 + r256(16 * 32) + r256(8 * ceil(P / 1024)) for the three models, the bit
    combined with every legal bit set of test_step_inputs_cpu.CONSTRUCTIONS; the two names resolve, 256-byte aligned, in that
    order behind everything else, and give GMVAE_E_NET without the bit; every other named offset stays where it was."""
    seen = set()
    for (model, y_inference, S, ge, *_), want in CONSTRUCTIONS:
        flags = _flags_of(L, y_inference, ge, want)
        K = 1 if model == "vae" else 10
        m = L.MODEL_IDS[model]
        d0 = L.make_dims(B, 784, 64, K, hidden, S=S, sched_flags=flags)
        d1 = L.make_dims(B, 784, 64, K, hidden, S=S, sched_flags=flags | L.OPT_CLIP_NORM)
        P, _ = L.param_count(d0, m)
        assert L.param_count(d1, m)[0] == P
        grow = 256 + r256(16 * L.LABEL_SLOTS) + r256(8 * ((P + 1023) // 1024))
        b0, b1 = L.workspace_bytes(d0, m), L.workspace_bytes(d1, m)
        assert b1 - b0 == grow, (model, flags, b0, b1)
        o_c, o_r = L.workspace_offset(d1, m, "clip_norm"), L.workspace_offset(d1, m, "grad_clip")
        # (behind every carved buffer; the size query itself may count more than the carve, the same with and without the bit)
        assert o_r == o_c + 256 and o_c % 256 == 0 and o_c <= b0 and o_c + grow <= b1
        for name in ("pixel_mask", "y_soft", "y_temperature", "obj_weights", "labels", "vs"):
            if L.lib.gmvae_workspace_offset(C.byref(d1), m, name.encode(), C.byref(C.c_uint64())) == 0:
                assert L.workspace_offset(d1, m, name) < o_c
        off = C.c_uint64()
        for name in (b"clip_norm", b"grad_clip"):
            assert L.lib.gmvae_workspace_offset(C.byref(d0), m, name, C.byref(off)) == E_NET
        for name in ("slabs", "qp", "z", "g", "dz"):
            assert L.workspace_offset(d0, m, name) == L.workspace_offset(d1, m, name)
        seen.add(model)
    assert seen == {"vae", "vae_gmp", "gmvae"}


def test_schedule_names(L):
    G, V = L.MODEL_GMVAE, L.MODEL_VAE
    name = lambda model, flags, **kw: L.step_schedule(L.make_dims(kw.pop("B", 1024), kw.pop("D", 784), kw.pop("Lz", 64),
                                                                  kw.pop("K", 10), kw.pop("hidden", (64,)), sched_flags=flags, **kw), model)
    Cn = L.OPT_CLIP_NORM
    assert name(G, 0) != "general"                                   # (the default sizes take a one-launch schedule without the bit)
    assert name(G, Cn) == "general+clip" and name(V, Cn, K=1, Lz=2) == "general+clip"
    assert name(L.MODEL_VAE_GMP, Cn) == "general+clip"
    assert name(G, Cn | L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS | L.GRAD_DREG, S=2) == "general+marginal_iw+labels+dreg+clip"
    assert name(G, Cn | L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH) == "general+weights+temp+st+clip"
    assert name(G, Cn | L.OBJ_PIXEL_MASK) == "general+mask+clip"
    planes = dict(B=8192, D=1024, Lz=64, hidden=(512, 512))
    assert name(G, 0, **planes).endswith("+planes")
    assert name(G, Cn, **dict(planes)) == "general+clip+planes"
    longest = name(G, Cn | L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS | L.GRAD_DREG, S=2, **dict(planes))
    assert len(longest) <= 47


def test_graph_constructors_refuse_more_records_than_slots(L):
    """n_steps = LABEL_SLOTS + 1 under the bit: GMVAE_E_DIMS from all three constructors, before anything is touched (every
    pointer is a host dummy); the profiles that stamp the fused optimizer launches refuse the bit."""
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    h = C.c_void_p()
    d = L.make_dims(16, 784, 8, 10, (64,), sched_flags=L.OPT_CLIP_NORM)
    r, G, n = C.byref(d), L.MODEL_GMVAE, L.LABEL_SLOTS + 1
    assert L.lib.gmvae_train_graph_create(r, G, p, n, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, C.byref(h)) == E_DIMS
    assert L.lib.gmvae_dp_graph_create(r, G, p, n, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None, C.byref(h)) == E_DIMS
    assert L.lib.gmvae_train_graph_create_pipeline(r, G, p, 100, p, p, n, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None,
                                                   C.byref(h)) == E_DIMS
    assert h.value is None
    nl = C.c_int()
    assert L.lib.gmvae_train_profile(r, G, p, p, p, p, p, p, 0, p, 1e-3, 1, 4, C.byref(nl), p, p, p, p, None) == E_DIMS
    assert L.lib.gmvae_dp_profile(r, G, p, p, p, p, p, p, 0, p, 1e-3, p, 1, p, 4, C.byref(nl), p, None) == E_DIMS


def test_evaluators_mask_the_bit(L):
    """gmvae_iw_bound* and gmvae_posterior_* size their workspaces as without the bit."""
    for kind, model, K in (("iw_bound", "vae", 1), ("iw_bound", "gmvae", 10), ("iw_bound_enum_y", "gmvae", 10),
                           ("posterior_y", "gmvae", 10), ("posterior_component", "vae_gmp", 10)):
        q = getattr(L, f"{kind}_workspace_bytes")
        m = L.MODEL_IDS[model]
        assert q(L.make_dims(16, 784, 8, K, (64,), S=5, sched_flags=L.OPT_CLIP_NORM), m) == \
            q(L.make_dims(16, 784, 8, K, (64,), S=5), m)


# ------------------------------------------------------------------ Python arguments
def test_check_clip_norm():
    from gmvae_amd.engine import check_clip_norm
    assert check_clip_norm(None) is None
    assert check_clip_norm(0.5) == 0.5 and check_clip_norm(3) == 3.0 and check_clip_norm(math.inf) == math.inf
    for bad in (0, 0.0, -1.0, math.nan, -math.inf, "x"):
        with pytest.raises(ValueError, match="clip_norm"):
            check_clip_norm(bad)


def test_engine_and_factories_take_the_argument():
    import inspect
    from gmvae_amd import gmvae, vae
    from gmvae_amd.engine import Engine
    assert inspect.signature(Engine.__init__).parameters["clip_norm"].default is None
    assert inspect.signature(gmvae.create_gmvae).parameters["clip_norm"].default is None
    assert inspect.signature(vae.create_vae).parameters["clip_norm"].default is None
    for name in ("set_clip_norm",):
        assert callable(getattr(Engine, name))


def test_check_args_refusals():
    from gmvae_amd import run_gmvae, runners
    p = run_gmvae.build_parser()
    assert p.parse_args([]).clip_norm == 0.0
    assert runners.clip_norm_of(p.parse_args([])) is None
    cfg = run_gmvae.check_args(p, p.parse_args(["--clip_norm", "0.5", "--model", "vae"]))
    assert runners.clip_norm_of(cfg) == 0.5
    assert runners.clip_norm_of(run_gmvae.check_args(p, p.parse_args(["--clip_norm", "inf"]))) == math.inf
    for bad in ("-1", "nan", "-inf"):                                 # (parsed as floats; check_args refuses them)
        assert p.parse_args([f"--clip_norm={bad}"]).clip_norm != 0
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args([f"--clip_norm={bad}"]))
