"""On the device: the launches a step runs -- the ordered names the measurement hooks report -- are the ones recorded in
tests/golden/launch_names_parent.json by the library as it stood before the schedule decision was folded into plan_step
(csrc/gmvae_hip.hip; profiles/schedule_plan_notes.md): an eager step at every gate corner, the steady-state step of a train
graph, the skinny schedule, forward-only passes, the data-parallel step, one general-schedule case per objective bit, the planes
and the switches that choose between two forms of one schedule.  One or a few steps per case."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("make_launch_names", os.path.join(GOLDEN, "make_launch_names.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen()
CASES = GEN.cases()
with open(os.path.join(GOLDEN, "launch_names_parent.json")) as _f:
    RECORDED = json.load(_f)
COMPARED = set()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_launches_are_the_recorded_ones(c):
    cus = GEN.compute_units()
    if c["edge"] and cus != RECORDED["compute_units"]:
        pytest.skip(f"the batch follows the compute-unit count: recorded on {RECORDED['compute_units']} units, this device has {cus}")
    want = RECORDED["names"][c["id"]]
    COMPARED.add(c["id"])
    assert GEN.run_case(c, cus) == want


def test_the_record_is_whole_and_no_fixed_case_was_left_out():
    """(runs behind the cases above)  Every case has a record, none of them an error or empty; every case whose batch does not
    follow the compute-unit count was compared; the record tells the forms of each schedule apart."""
    names = RECORDED["names"]
    assert set(names) == {c["id"] for c in CASES}
    assert all(isinstance(v, list) and v for v in names.values()), [k for k, v in names.items() if not (isinstance(v, list) and v)]
    assert {c["id"] for c in CASES if not c["edge"]} <= COMPARED
    seen = {n for v in names.values() for n in v}
    assert {"mega_fwd_bwd", "mega3_step", "mega3v_step", "mega2_fwd_bwd", "dw_adam", "finalize_adam", "mega3_grads", "dw_grads",
            "evalf_rows", "evalf_rows_v", "chain_fwd", "sk_dw", "sk_dw_adam", "finalize_grads_ss", "pmask_rows",
            "split_planes"} <= seen, seen
    assert names["train:train-gmvae-B1024"] == ["mega3_step"] and names["train-NO_FUSE"] == ["mega2_fwd_bwd", "dw_adam"]
    assert names["train-NO_FL"] != names["train-NO_FUSE"] and names["train-SCHED_SAFE"] != names["train:train-gmvae-B1024"]
    assert names["fwd-pairs-B8064"] != names["fwd-pairs-B8192"]
    assert "split_planes_rw" in names["planes-S4"] and "split_planes" in names["fwd-pairs-B8192"]
