"""No GPU: tests/gate_corners.py against the size gates of csrc/gmvae_hip.hip as they stand (gmvae_step_schedule and
gmvae_workspace_bytes need no device).  A change of a gate constant -- kSkMaxB, GMP_PARTS, an LDS budget, a bound on L, K or H --
fails here first: move the corner to the new edge in the table, keep the old shape as its `outside_of` case."""
import dataclasses

import pytest

import gate_corners as G
import oracle as O


def _lib():
    from gmvae_amd import _lib
    return _lib


def _dims(L, c, d=None, B=None):
    d = d or c.d
    return L.make_dims(B or c.B, d.D, d.L, d.K, d.hidden, S=d.S)


def _schedule(monkeypatch, c, d=None, B=None):
    L = _lib()
    for k in G.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    return L.step_schedule(_dims(L, c, d, B), O.MODEL_NAMES[c.model])


# (mega2v_ok and evalf_ok read the device's compute-unit count: tests/test_gate_corners.py asserts those corners)
NAMED = [c for c in G.CORNERS if c.edge is None]


@pytest.mark.parametrize("c", NAMED, ids=[c.id for c in NAMED])
def test_corner_takes_the_schedule_the_table_names(c, monkeypatch):
    assert _schedule(monkeypatch, c) == c.sched


@pytest.mark.parametrize("c", G.CORNERS, ids=[c.id for c in G.CORNERS])
def test_workspace_is_sized_at_every_corner(c):
    L = _lib()
    assert L.workspace_bytes(_dims(L, c), O.MODEL_NAMES[c.model]) > 0


OUTSIDE = [c for c in G.CORNERS if c.outside_of]


@pytest.mark.parametrize("c", OUTSIDE, ids=[c.id for c in OUTSIDE])
def test_first_shape_outside_a_gate_falls_to_another_schedule(c, monkeypatch):
    inside = G.BY_ID[c.outside_of]
    assert c.sched != inside.sched and c.env == inside.env and c.model == inside.model and c.kind == inside.kind
    if c.edge is None:
        assert _schedule(monkeypatch, c) != _schedule(monkeypatch, inside)
    # one step past the gate in ONE dimension, everything else equal
    a, b = dataclasses.asdict(c.d), dataclasses.asdict(inside.d)
    moved = [k for k in a if a[k] != b[k]] + (["B"] if c.B != inside.B else [])
    assert len(moved) == 1, moved


@pytest.mark.parametrize("cid,dL", [("mega-gmvae-lds-edge", 2), ("mega-vae-lds-edge", 2), ("mega-vae_gmp-lds-edge", 2), ("fused-lds-edge", 8),
                                    ("mega-gmvae-L128", None), ("mega-vae_gmp-L128", None), ("fused-L128", None)])
def test_lds_edge_corners_lie_on_the_admitted_frontier(cid, dL, monkeypatch):
    """The next latent size the gate's stride allows and the next K are both refused."""
    c = G.BY_ID[cid]
    assert _schedule(monkeypatch, c) == c.sched
    if dL:
        assert _schedule(monkeypatch, c, dataclasses.replace(c.d, L=c.d.L + dL)) != c.sched
    if c.model != "vae":
        assert _schedule(monkeypatch, c, dataclasses.replace(c.d, K=c.d.K + 1)) != c.sched


def test_batch_edges_at_256_compute_units():
    """batch_on restates the two predicates that read the compute-unit count; the table's literal B is its value at 256."""
    for c in G.CORNERS:
        if c.edge:
            assert G.batch_on(c, 256) == c.B, c.id
    e = G.BY_ID["evalf-gmvae-NB"]
    assert G.batch_on(e, 304) == 304 * G.EV_NB and G.batch_on(e, 2000) == 1024 * G.EV_NB
    v = G.BY_ID["train-vae-panels37"]
    assert G.batch_on(v, 128) == 18 * G.PANEL + 1 and G.batch_on(v, 304) == 36 * G.PANEL + 1


def test_table_is_not_hollow():
    inside = [c for c in G.CORNERS if not c.outside_of]
    names = {c.sched for c in inside}
    assert {"mega", "mega2", "mega2v", "fused", "skinny", "evalf"} <= names, names
    assert any(c.sched == "general" for c in G.CORNERS)
    assert any(c.d.D > 904 and c.sched == "mega" for c in inside)
    assert any(c.d.D > 904 and c.sched == "skinny" for c in inside)
    assert any(c.d.L == 128 and c.sched == "mega" for c in inside)
    assert any(c.d.L == 128 and c.sched == "fused" for c in inside)
    assert any(c.d.L == 256 and c.sched == "skinny" for c in inside)
    assert any(c.d.hidden == (16,) and c.sched == "mega" for c in inside)
    for m in G.MODELS:                       # all three models on the one-launch and the skinny schedules, and forward only
        assert {"mega", "skinny", "evalf"} <= {c.sched for c in inside if c.model == m}, m
    for sw in (k for c in G.CORNERS for k, _ in c.env):
        assert sw in G.SWITCHES
