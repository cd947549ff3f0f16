"""The seven fp64 statements (tests/*_ref.loss_and_grads, adapters onto tests/objective_ref.py) against what they returned before
they shared one forward pass: tests/golden/objective_ref_parent.json, written by tests/golden/make_objective_ref_golden.py at
the parent commit -- every case table of the seven modules and their device tests, and each optional switch at least once.

The operations and their order are meant to be unchanged, so the expected difference is 0.  Allowed: 1e-12 of the tensor's
recorded largest magnitude for each of its three numbers (sum, largest magnitude, dot product with a fixed-seed vector), 1e-12 of
max(|value|, 1) for a scalar -- fp64 reassociation of sums of a few thousand terms is ~1e-13, and the gates these statements
serve are at 1e-4.  The largest difference seen is printed (profiles/objective_ref_refactor_notes.md records it)."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-12

_spec = importlib.util.spec_from_file_location("make_objective_ref_golden", os.path.join(GOLDEN, "make_objective_ref_golden.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)
with open(os.path.join(GOLDEN, "objective_ref_parent.json")) as _f:
    PARENT = GEN.unpack(json.load(_f))


@pytest.fixture(scope="module")
def records():
    return GEN.records()


def test_the_file_holds_every_record(records):
    assert list(records) == list(PARENT) and len(PARENT) >= 80


@pytest.mark.parametrize("rid", list(PARENT))
def test_statement_is_the_parents(records, rid):
    got, want = GEN.digest_of(rid, records[rid]), PARENT[rid]
    assert list(got) == list(want)                                   # every key of C and of g, in the parent's order
    worst = 0.0
    for k, w in want.items():
        v = got[k]
        if w is None or v is None:
            assert v is None and w is None, k
        elif isinstance(w, list):
            for a, b, what in zip(v, w, ("sum", "max", "dot")):
                err = abs(a - b) / max(w[1], 1e-300)
                worst = max(worst, err)
                assert abs(a - b) <= RTOL * w[1], (rid, k, what, a, b)
        else:
            err = abs(v - w) / max(abs(w), 1.0)
            worst = max(worst, err)
            assert abs(v - w) <= RTOL * max(abs(w), 1.0), (rid, k, v, w)
    print(f"{rid}: largest difference {worst:.3e} of its bound's scale")
