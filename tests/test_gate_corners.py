"""-m gpu: every corner of tests/gate_corners.py on the schedule the table names, against the fp64 oracle.

step   hip_util.compare_step at test_step_matches_oracle's preparation (biases drawn at 0.05, oracle.make_inputs) and its gates:
       the ELBO and each term at 1e-4 (BASELINE.json north_star), every gradient tensor at 1e-4 of its maximum, the ReLU-mask rule
evalf  gmvae_forward's rows and tail against oracle.forward at test_forward_outputs' tolerances; that the one-launch evaluation
       ran (or did not) shows in the bits of GMVAE_NO_EVALF=1's rows
train  three steps of a train graph through test_timed_path.trajectory_case, at that file's gates"""
import re

import numpy as np
import pytest
import torch

import gate_corners as G
import oracle as O

pytestmark = pytest.mark.gpu

REPORT = {}            # corner id -> (schedule, worst error / gate, ReLU units taken from the device): test_gate_corner_margins_report


def _of_kind(kind):
    cs = [c for c in G.CORNERS if c.kind == kind]
    return pytest.mark.parametrize("c", cs, ids=[c.id for c in cs])


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _set_env(monkeypatch, c):
    for k in G.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)


@_of_kind("step")
def test_step_at_gate_corner_matches_oracle(c, monkeypatch):
    import hip_util as H
    from gmvae_amd import _lib as L
    _set_env(monkeypatch, c)
    model, d, B = O.MODEL_NAMES[c.model], c.d, c.B
    sched = L.step_schedule(H.dims_of(d, B), model)
    assert sched == c.sched
    rng = np.random.default_rng(B)
    p = O.init_params(model, d, rng)
    for k in p:
        if k.endswith("/b"):
            p[k] = rng.normal(0, 0.05, p[k].shape)
    x, eps, u = O.make_inputs(d, B, model)
    n_m, n_f = len(H.MARGINS), len(H.FLIPS)
    try:
        H.compare_step(model, d, p, x, eps, u)
    finally:
        REPORT[c.id] = (sched, max((v for _, v in H.MARGINS[n_m:]), default=float("nan")), len(H.FLIPS) - n_f)


@_of_kind("evalf")
def test_forward_at_evalf_batch_edge_matches_oracle(c, monkeypatch):
    import hip_util as H
    _set_env(monkeypatch, c)
    model, d, B = O.MODEL_NAMES[c.model], c.d, G.batch_on(c, _cus())
    x, eps, u = O.make_inputs(d, B, model)
    flat = O.pack(model, d, O.init_params(model, d, np.random.default_rng(5)), np.float32)
    Cc = O.forward(model, d, O.unpack(model, d, flat.astype(np.float64)), x, eps, u)
    tail, rows, _ = H.forward_call(model, d, flat, x, 1, eps, u)
    np.testing.assert_allclose(rows[:, 0], Cc["logpx"], rtol=1e-5)
    np.testing.assert_allclose(rows[:, 3], Cc["logw"], rtol=1e-5)
    assert tail[0] / B == pytest.approx(Cc["loss"], rel=1e-5)
    monkeypatch.setenv("GMVAE_NO_EVALF", "1")
    rows32 = H.forward_call(model, d, flat, x, 1, eps, u)[1]
    # evalf.hpp multiplies bf16 pieces, the schedules behind it fp32 tiles: the same bits mean the same kernels.  (An inference,
    # not a query: it assumes the schedules behind evalf give the same bits on two runs of the same inputs.  If they ever do
    # not, an "other" corner reads as "evalf" and this fails loudly; it cannot pass wrongly for an "evalf" corner's gate.)
    took = "other" if np.array_equal(rows[:, 0], rows32[:, 0]) else "evalf"
    REPORT[c.id] = (took, float(np.abs(rows[:, 3] / Cc["logw"] - 1).max() / 1e-5), 0)
    assert took == c.sched


@_of_kind("train")
def test_train_graph_at_gate_corner_matches_oracle_trajectory(c, monkeypatch, capfd):
    import test_timed_path as T
    from gmvae_amd import _lib as L
    _set_env(monkeypatch, c)
    model, d, B = O.MODEL_NAMES[c.model], c.d, G.batch_on(c, _cus())
    sched = L.step_schedule(L.make_dims(B, d.D, d.L, d.K, d.hidden), model)
    assert sched == c.sched
    monkeypatch.setenv("GMVAE_TRACE", "1")       # one line per captured mega_fwd_bwd call: first_layer_inside
    n_g, n_f = len(T.GRAD_STATS), len(T.FLIPS)
    try:
        T.trajectory_case(c.model, d.D, d.L, d.K, d.hidden, B, 3)
    finally:
        REPORT[c.id] = (sched, max((e for *_, e in T.GRAD_STATS[n_g:]), default=float("nan")) / 1e-4, len(T.FLIPS) - n_f)
    if c.fl_inside is not None:
        inside = [int(v) for v in re.findall(r"mega_fwd_bwd: model \d+ B \d+ first_layer_inside (\d)", capfd.readouterr().err)]
        assert inside and max(inside) == c.fl_inside, inside


def test_gate_corner_margins_report():
    """Not a gate: what the corners above measured in this process (file order, run with -s), per corner -- the schedule, the
    worst error over its gate and the ReLU units taken from the device.  The source of the table in
    profiles/gate_corners_notes.md; it prints only the corners that ran before it."""
    print()
    for cid, (sched, margin, flips) in REPORT.items():
        print(f"[gate corner] {cid:28s} {sched:8s} worst error / gate {margin:.3f}  ReLU flips {flips}")
