"""The per-step inputs (engine.STEP_INPUTS: labels, weights, temperature, mask) through the eager fallback of a refused
data-parallel graph: the one driver that feeds row i of every input through slot 0, on each input's smallest engine case."""
import numpy as np
import pytest

import pmask_ref as PR
from hip_util import drop_comm, need_rccl
import test_pmask
import test_semisup
import test_wobj
import test_ytemp
import wobj_ref as WR
import ytemp_ref as TR

pytestmark = pytest.mark.gpu

LR = 1e-3
B = 16
N = 3


def _labels_case(seed):
    import torch
    d = test_semisup.CASES["a"][0]
    kw = dict(n_samples=2, semi_supervised=True, sup_weight=test_semisup.ALPHA)
    rows = test_semisup._three_label_sets(d.K, B).to(torch.int32)
    return d, (lambda: test_semisup._engine(d, seed, **kw)), rows, (lambda a, x, r: a.train_step(x, lr=LR, y_observed=r)), None


def _weights_case(seed):
    import torch
    d = WR.CASES["gumbel"][2]
    own = (0.5, 0.75, 0.1)
    rows = torch.tensor([test_wobj.ROWS8[t + 2] + (0.0,) for t in range(N)], dtype=torch.float32).cuda()

    def eager(a, x, r):
        a.set_objective_weights(*r[:3].tolist())
        return a.train_step(x, lr=LR)

    def unchanged(b):
        assert torch.equal(b._objw_dev.cpu(), torch.tensor(own + (0.0,), dtype=torch.float32)) and b.obj_weights == own
    return d, (lambda: test_wobj._engine("gumbel", seed, kl_weight=own[0], y_weight=own[1], y_free_nats=own[2])), rows, eager, unchanged


def _temperature_case(seed):
    import torch
    d = TR.CASES["K7-weights"][0]
    rows = torch.tensor(test_ytemp.ROWS[0], dtype=torch.float32).cuda()

    def eager(a, x, r):
        a.set_temperature(r.item())
        return a.train_step(x, lr=LR)

    def unchanged(b):
        assert b.temperature == 1.5 and b.dims(B).temperature == 1.5 and torch.equal(b._tau_dev.cpu(), torch.tensor([1.5]))
    return d, (lambda: test_ytemp._engine(seed, "relaxed")), rows, eager, unchanged


def _mask_case(seed):
    d = PR.CASES["gumbel"].d
    _, rows = test_pmask._batches(d, B, N, seed)
    return d, (lambda: test_pmask._engine("gumbel", seed)), rows, (lambda a, x, r: a.train_step(x, lr=LR, mask=r)), None


CASES = {"y_observed": _labels_case, "obj_weights": _weights_case, "y_temperature": _temperature_case, "pixel_mask": _mask_case}


@pytest.mark.parametrize("name", list(CASES))
def test_eager_fallback_of_a_refused_dp_graph_reads_one_row_per_step(name, monkeypatch):
    """capture_train_step(all_reduce=True) where the library refuses the data-parallel graph: replay() runs the steps one by
    one through gmvae_dp_step, row i of replay.<name> passing through slot 0.  Same bits -- parameters, both moments, every
    step's tail -- as eager train_steps given those rows; afterwards replay.<name> still holds the three rows and the engine's
    own current weights / temperature are what they were."""
    import torch
    from gmvae_amd import _lib as L
    from gmvae_amd.engine import STEP_INPUTS
    need_rccl()
    d, make, rows, eager, unchanged = CASES[name](17)
    assert rows.shape[0] == N and len({tuple(r.flatten().tolist()) for r in rows.cpu()}) == N      # (three distinct rows)
    xs = torch.from_numpy((np.random.default_rng(12).random((N, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = make(), make()
    assert a.step_inputs == b.step_inputs == tuple(inp.option for inp in STEP_INPUTS if inp.replay == name)
    b.enable_rccl()
    try:
        tails = [eager(a, xs[t], rows[t]).clone() for t in range(N)]
        monkeypatch.setattr(L.lib, "gmvae_dp_graph_create", lambda *args: -2)      # the refusal: no graph, no handle
        sb, rb = b.capture_train_step(B, lr=LR, all_reduce=True, n_steps=N)
        assert b.dp_mode == "rccl-eager-c"
        for inp in STEP_INPUTS:                                                    # the engine's one input, and no other
            assert (getattr(rb, inp.replay) is not None) == (inp.replay == name)
        view = getattr(rb, name)
        assert view.shape == rows.shape and view.dtype == rows.dtype
        sb.copy_(xs)
        view.copy_(rows)
        rb()
        torch.cuda.synchronize()
        assert a.global_step == b.global_step == N
        for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
            assert torch.equal(u.detach(), v.detach())
        assert torch.equal(rb.tail_log, torch.stack(tails)) and bool(torch.isfinite(rb.tail_log).all())
        assert torch.equal(view, rows)                                             # row 0 restored after the eager calls
        if unchanged is not None:
            unchanged(b)
    finally:
        drop_comm(b)
