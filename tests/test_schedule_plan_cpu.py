"""No GPU: the schedule a training step takes -- gmvae_step_schedule's string or return code -- and gmvae_workspace_bytes are the
ones recorded in tests/golden/schedule_table.json by the library as it stood before the decision was folded into plan_step
(csrc/gmvae_hip.hip; profiles/schedule_plan_notes.md): every gate corner x every bit and pair of bits x every switch."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORDS = {"general", "mega", "mega2", "mega2v", "skinny", "fused"}
SUFFIXES = {"marginal", "marginal_iw", "labels", "weights", "temp", "st", "mask", "dreg", "clip", "planes"}


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_schedule_table", os.path.join(GOLDEN, "make_schedule_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "schedule_table.json")) as f:
        return json.load(f)


def _answers(case):
    s = case["sched"]
    return s if isinstance(s, list) else [s]


def test_every_schedule_and_size_is_the_recorded_one(L, gen, golden):
    now = gen.table(L)
    assert now["variants"] == golden["variants"] and now["plane_variants"] == golden["plane_variants"]
    assert len(now["cases"]) == len(golden["cases"]) >= 1000
    for got, want in zip(now["cases"], golden["cases"]):
        assert got == want


def test_table_covers_every_gate_corner_without_a_device_edge(gen, golden):
    import gate_corners as G
    ids = {c["id"] for c in golden["cases"]}
    assert ids == {c.id for c in G.CORNERS if c.edge is None} | {e[0] for e in gen.EXTRA}
    assert {v[1].get(k) for v in gen.VARIANTS for k in G.SWITCHES} >= {"1"} and len(gen.VARIANTS) >= len(G.SWITCHES) + 3
    for sw in G.SWITCHES + ("GMVAE_NO_PLANES",):
        assert any(v[1] == {sw: "1"} for v in gen.VARIANTS), sw
    assert any(v[2] == 1 for v in gen.VARIANTS)              # GMVAE_SCHED_SAFE
    assert any(v[1].get("GMVAE_PLANES_MINROWS") == "128" for v in gen.PLANE_VARIANTS)


def test_table_is_not_hollow(L, golden):
    """Every word and every +suffix of the report occurs; every switch changes some answer; for each bit that only the general
    schedule implements, some shape takes mega, skinny or fused without the bit and the general schedule with it."""
    words, suffixes = set(), set()
    for c in golden["cases"]:
        for a in _answers(c):
            if isinstance(a, str):
                head, *rest = a.split("+")
                words.add(head)
                suffixes |= set(rest)
    assert words == WORDS and suffixes == SUFFIXES
    assert any(isinstance(a, int) and a < 0 for c in golden["cases"] for a in _answers(c))      # a refused combination
    nv = len(golden["variants"])
    for i in range(1, nv):                                    # variant i differs from no switch somewhere
        if golden["variants"][i] not in ("NO_EVALF", "NO_PLANES"):      # (a forward-only gate; needs the forced rows, below)
            assert any(isinstance(c["sched"], list) and c["sched"][i] != c["sched"][0] for c in golden["cases"]), golden["variants"][i]
    forced = [c["sched"] for c in golden["cases"] if isinstance(c["sched"], list) and len(c["sched"]) > nv]
    assert any(s[nv] != s[0] and s[nv].endswith("+planes") for s in forced)      # GMVAE_PLANES_MINROWS=128
    assert any(s[nv + 1] != s[nv] for s in forced)                               # ... and GMVAE_NO_PLANES on top of it
    plain = {c["id"]: _answers(c)[0] for c in golden["cases"] if c["flags"] == 0}
    for bit in (L.GRAD_DREG, L.OBJ_WEIGHTS, L.Y_TEMP_DEV, L.Y_STRAIGHT_THROUGH, L.OBJ_PIXEL_MASK, L.OPT_CLIP_NORM,
                L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW):
        moved = {plain[c["id"]] for c in golden["cases"]
                 if c["flags"] == bit and isinstance(_answers(c)[0], str) and _answers(c)[0].startswith("general")}
        assert moved & {"mega", "mega2", "mega2v", "skinny", "fused"}, bit
    assert all(isinstance(c["bytes"], int) and c["bytes"] > 0 or isinstance(_answers(c)[0], int) for c in golden["cases"])
