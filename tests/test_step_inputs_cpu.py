"""The per-step inputs (labels, weights, temperature, mask) without a device: the workspace layout is the recorded one, byte for
byte, and engine.STEP_INPUTS -- the one table the Python side reads them from -- agrees with what the library carves."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_NET = -5          # include/gmvae_hip.h GMVAE_E_NET: gmvae_workspace_offset's answer for a name these dims do not carve


def r256(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_step_inputs_layout", os.path.join(GOLDEN, "make_step_inputs_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "step_inputs_layout.json")) as f:
        return json.load(f)


def test_layout_is_the_recorded_one(L, gen, golden):
    """gmvae_workspace_bytes and every named offset, over the whole grid, equal the file recorded before the fold."""
    assert golden["label_slots"] == L.LABEL_SLOTS == 32
    assert golden["names"] == gen.NAMES
    now = gen.layout(L)
    assert len(now["cases"]) == len(golden["cases"]) >= 100
    for got, want in zip(now["cases"], golden["cases"]):
        assert got == want, {k: v for k, v in want.items() if k not in ("offsets", "bytes")}


def test_grid_covers_every_legal_combination(L, golden):
    """The three models, the four batch sizes, both sample counts, the H = 512 sizes, and every subset of the four bits that
    some entry point accepts: none, each bit alone, weights + temperature."""
    from gmvae_amd.engine import STEP_INPUTS
    cases = golden["cases"]
    assert {c["model"] for c in cases} == {"vae", "vae_gmp", "gmvae"}
    assert {c["B"] for c in cases} == {1, 16, 100, 1024} and {c["S"] for c in cases} == {1, 3}
    assert {tuple(c["hidden"]) for c in cases} == {(64,), (512,)}
    bits = 0
    for inp in STEP_INPUTS:
        bits |= inp.bit
    W, T = L.OBJ_WEIGHTS, L.Y_TEMP_DEV
    assert {c["flags"] & bits for c in cases} == {0, W | T} | {inp.bit for inp in STEP_INPUTS}
    # every other subset is refused (GMVAE_E_DIMS) whatever else the dims carry
    for sub in range(bits + 1):
        if sub & ~bits or sub in (0, W | T) or sub in [inp.bit for inp in STEP_INPUTS]:
            continue
        for extra in (0, L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW):
            d = L.make_dims(16, 784, 64, 10, (64,), sched_flags=sub | extra)
            with pytest.raises(L.GmvaeError, match="GMVAE_E_DIMS"):
                L.workspace_bytes(d, L.MODEL_GMVAE)


def test_table_agrees_with_the_library(L, golden):
    """For every entry of STEP_INPUTS and every case: the region resolves exactly when the bit is set (GMVAE_E_NET otherwise),
    its slots are the C side's -- pad4(B) * 4, 16, 4 and r256(B D) bytes apart -- and LABEL_SLOTS of them, rounded up to 256
    bytes, reach exactly to the next region of the recorded layout: "sup_weight" behind the labels, "rwk" behind the weight
    rows, "y_soft" behind the temperatures under GMVAE_Y_STRAIGHT_THROUGH.  Where nothing named follows (the temperatures
    without that bit; the masks, followed by x~, the held-out partials and the counts: include/gmvae_hip.h), the workspace
    grows by exactly that much over the recorded case without the bit.  (Measured as growth, not against the total: the size
    query counts the one-launch schedules' first-layer slabs twice at the sizes that take both, the same with and without
    the bit.)"""
    from gmvae_amd.engine import STEP_INPUTS
    assert [inp.region for inp in STEP_INPUTS] == ["labels", "obj_weights", "y_temperature", "pixel_mask"]
    assert [inp.replay for inp in STEP_INPUTS] == ["y_observed", "obj_weights", "y_temperature", "pixel_mask"]
    assert [inp.bit for inp in STEP_INPUTS] == [L.OBJ_LABELS, L.OBJ_WEIGHTS, L.Y_TEMP_DEV, L.OBJ_PIXEL_MASK]
    at = {n: i for i, n in enumerate(golden["names"])}
    key = lambda c, flags: (c["model"], c["B"], c["D"], c["L"], c["K"], tuple(c["hidden"]), c["S"], flags)
    size_of = {key(c, c["flags"]): c["bytes"] for c in golden["cases"]}
    checked = {inp.region: 0 for inp in STEP_INPUTS}
    for c in golden["cases"]:
        B, D, S = c["B"], c["D"], c["S"]
        c_strides = {"labels": (B + 3) // 4 * 4 * 4, "obj_weights": 16, "y_temperature": 4, "pixel_mask": r256(B * D)}
        off = lambda name: c["offsets"][at[name]]
        for inp in STEP_INPUTS:
            if not c["flags"] & inp.bit:
                assert off(inp.region) == E_NET, (c, inp.region)
                continue
            stride = inp.stride(B, D) * inp.dtype.itemsize
            assert stride == c_strides[inp.region], (c, inp.region)
            assert off(inp.region) >= 0 and off(inp.region) % 256 == 0
            region = r256(stride * L.LABEL_SLOTS)
            behind = {"labels": "sup_weight", "obj_weights": "rwk",
                      "y_temperature": "y_soft" if c["flags"] & L.Y_STRAIGHT_THROUGH else None, "pixel_mask": None}[inp.region]
            if behind is not None:
                assert off(inp.region) + region == off(behind), (c, inp.region)
            else:
                tail = r256(B * D) + r256(4 * B * S * ((D + 31) // 32)) + r256(8 * B) if inp.region == "pixel_mask" else 0
                assert c["bytes"] - size_of[key(c, c["flags"] & ~inp.bit)] == region + tail, (c, inp.region)
                assert off(inp.region) + region + tail <= c["bytes"]
            n = 1
            for s in inp.shape(B, D):
                n *= s
            assert n <= inp.stride(B, D)                     # (the visible part of a slot lies inside the slot)
            checked[inp.region] += 1
    assert min(checked.values()) >= 10, checked


def test_constructor_stores_what_the_table_reads():
    """Every entry's option is an argument of Engine(...) that the constructor stores under that name, and its engine-held
    tensor is an attribute the constructor creates: what STEP_INPUTS reads with getattr.  (Read from the constructor's source:
    constructing an engine needs a device; tests/test_step_inputs.py holds a constructed engine's step_inputs to its option.)"""
    import inspect
    from gmvae_amd.engine import STEP_INPUTS, Engine
    params = inspect.signature(Engine.__init__).parameters
    src = inspect.getsource(Engine.__init__)
    for inp in STEP_INPUTS:
        assert inp.option in params and params[inp.option].default is False
        assert f"self.{inp.option} = bool({inp.option})" in src
        assert (inp.held is None) != (inp.arg is None)
        if inp.held:
            assert f"self.{inp.held} = torch." in src and f"if self.{inp.option}:" in src
        else:
            assert inp.check is not None and inp.absent is not None
            for entry in (Engine.step, Engine.forward, Engine.dp_step, Engine.train_step, Engine.loss):
                assert inspect.signature(entry).parameters[inp.arg].default is None


CONSTRUCTIONS = [   # (model, y_inference, n_samples, grad_estimator, semi_supervised, weighted_objective, temperature_on_device,
                    #  pixel_mask) -> Engine.step_inputs
    (("gmvae", "gumbel", 1, "standard", False, False, False, False), ()),
    (("vae", "gumbel", 3, "dreg", False, False, False, False), ()),
    (("gmvae", "marginal", 1, "standard", True, False, False, False), ("semi_supervised",)),
    (("gmvae", "marginal_iw", 3, "dreg", True, False, False, False), ("semi_supervised",)),
    (("gmvae", "gumbel", 1, "standard", False, True, False, False), ("weighted_objective",)),
    (("gmvae", "marginal", 1, "standard", False, True, False, False), ("weighted_objective",)),
    (("vae", "gumbel", 1, "standard", False, True, False, False), ("weighted_objective",)),
    (("vae_gmp", "gumbel", 1, "standard", False, True, False, False), ("weighted_objective",)),
    (("gmvae", "gumbel", 3, "standard", False, False, True, False), ("temperature_on_device",)),
    (("gmvae", "gumbel", 1, "standard", False, True, True, False), ("weighted_objective", "temperature_on_device")),
    (("gmvae", "gumbel", 3, "standard", False, False, False, True), ("pixel_mask",)),
    (("vae", "gumbel", 1, "standard", False, False, False, True), ("pixel_mask",)),
    (("vae_gmp", "gumbel", 3, "standard", False, False, False, True), ("pixel_mask",)),
]


@pytest.mark.parametrize("args,want", CONSTRUCTIONS, ids=["-".join(map(str, a[:4])) + "-" + ("+".join(w) or "none") for a, w in CONSTRUCTIONS])
def test_engine_step_inputs(L, args, want):
    """Engine.step_inputs for every legal combination of the constructor's options: the argument side of the constructor (its
    four check_* functions, no device) followed by the property on the options it stores."""
    from gmvae_amd import engine as E
    model, y_inference, S, ge, sup, wobj, ytd, pmk = args
    E.check_pixel_mask(model, y_inference, ge, sup, wobj, ytd, "relaxed", pmk)
    E.check_y_head(model, y_inference, 1.0, ytd, "relaxed")
    E.check_semi_supervised(model, y_inference, sup, 1.0)
    E.check_weighted_objective(model, y_inference, S, ge, sup, wobj, 1.0, 1.0, 0.0)
    eng = E.Engine.__new__(E.Engine)
    eng.semi_supervised, eng.weighted_objective, eng.temperature_on_device, eng.pixel_mask = sup, wobj, ytd, pmk
    assert eng.step_inputs == want
    assert [inp.option for inp in E.STEP_INPUTS] == ["semi_supervised", "weighted_objective", "temperature_on_device", "pixel_mask"]
    # the library accepts the dims such an engine builds
    flags = {"gumbel": 0, "marginal": L.OBJ_MARGINAL_Y, "marginal_iw": L.OBJ_MARGINAL_Y_IW}[y_inference]
    flags |= L.GRAD_DREG if ge == "dreg" else 0
    for inp in E.STEP_INPUTS:
        flags |= inp.bit if inp.option in want else 0
    K = 1 if model == "vae" else 10
    assert L.workspace_bytes(L.make_dims(16, 784, 64, K, (64,), S=S, sched_flags=flags), L.MODEL_IDS[model]) > 0


def test_graph_constructors_refuse_more_steps_than_slots(L):
    """n_steps = LABEL_SLOTS + 1 with any of the four bits: GMVAE_E_DIMS from both graph constructors, before anything is
    touched (every pointer is a host dummy); the pipeline graph refuses the bits at any n_steps."""
    import ctypes as C
    from gmvae_amd.engine import STEP_INPUTS
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    h = C.c_void_p()
    for inp in STEP_INPUTS:
        flags = inp.bit | (L.OBJ_MARGINAL_Y if inp.bit == L.OBJ_LABELS else 0)
        d = L.make_dims(16, 784, 8, 10, (64,), sched_flags=flags)
        r = C.byref(d)
        G = L.MODEL_GMVAE
        assert L.lib.gmvae_train_graph_create(r, G, p, L.LABEL_SLOTS + 1, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None,
                                              C.byref(h)) == -2
        assert L.lib.gmvae_dp_graph_create(r, G, p, L.LABEL_SLOTS + 1, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, None,
                                           C.byref(h)) == -2
        assert L.lib.gmvae_train_graph_create_pipeline(r, G, p, 100, p, p, 2, p, p, p, p, p, 0, p, 1e-3, 0.9, 0.999, 1e-8, None,
                                                       C.byref(h)) == -2
    assert h.value is None
