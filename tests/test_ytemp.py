"""The device-side Gumbel-softmax temperature and the straight-through y (GMVAE_Y_TEMP_DEV, GMVAE_Y_STRAIGHT_THROUGH) on the
device: the step through the C ABI on explicit noise against the fp64 statement (tests/ytemp_ref.py) at the project's gates --
loss at 1e-4 relative, nll / kl / nent each relative to itself, every gradient tensor at 1e-4 of its own max -- the bit identity
with the step without the bit, gmvae_forward, the train and data-parallel graphs, the refusals and the runner.

Low temperature, tau = 0.1 (profiles/ytemp_notes.md): the step WITHOUT the bits at dims->temperature = 0.1 was measured against
the statement on the parent commit on these cases -- per case the worst gradient error 1.1e-06 / 9.4e-07 / 2.2e-06 / 2.0e-06 of the
tensor's max, the worst loss error 1.2e-07 relative, all below 1e-4 -- so the straight-through step at tau = 0.1, which feeds the same backward kernel the same y_soft, is held to the
project's 1e-4 too."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import oracle as O
import ytemp_ref as TR
from hip_util import _L, check_grads, dev, dims_of, drop_comm, hip_step, need_rccl, tail_gates, write_inputs

pytestmark = pytest.mark.gpu

LR = 1e-3
GM = O.MODEL_GMVAE
_REF = {}          # (case, tau, straight-through) -> the fp64 statement's (C, g): computed once, shared, left unchanged


def _ref(name, tau, st):
    key = (name, float(tau), bool(st))
    if key not in _REF:
        d, p32, flat, x, eps, u = TR.setup(name)
        _REF[key] = TR.loss_and_grads(d, p32, x, eps, u, tau, straight_through=st, weights=TR.case_weights(name))
    return _REF[key]


def _cdims(name, B, temp_dev, st, temperature, d=None):
    L = _L()
    d = d or TR.CASES[name][0]
    cd = dims_of(dataclasses.replace(d, temperature=temperature), B)
    cd.sched_flags = ((L.Y_TEMP_DEV if temp_dev else 0) | (L.Y_STRAIGHT_THROUGH if st else 0) |
                      (L.OBJ_WEIGHTS if TR.case_weights(name) else 0))
    return cd


def _inputs(cd, name, tau):
    """The caller's regions: slot 0 of the temperatures (the other slots stay 0: a kernel reading another slot gives NaN) and of
    the weight rows."""
    L = _L()
    inputs = {}
    if cd.sched_flags & L.Y_TEMP_DEV:
        inputs["y_temperature"] = [tau]
    if cd.sched_flags & L.OBJ_WEIGHTS:
        inputs["obj_weights"] = list(TR.case_weights(name)) + [0.0]
    return inputs


def ystep(name, tau, st, temp_dev=True, temperature=1.0, case=None, row0=0):
    """One gmvae_step of a case at row0.  temp_dev: slot 0 holds tau and dims->temperature the decoy `temperature`; else
    dims->temperature = tau.  case: (Dims, p32, flat, x, eps, u) in TR.setup's form where they are not the named case's own
    (tests/test_shards.py; `name` then only says whether the weights go with it).
    Returns (grad sums [P] float64, tail [8], the step's ReLU masks, the workspace, its dims)."""
    d, p32, flat, x, eps, u = case or TR.setup(name)
    temperature = temperature if temp_dev else tau
    cd = _cdims(name, x.shape[0], temp_dev, st, temperature, d)
    return hip_step(GM, dataclasses.replace(d, temperature=temperature), flat, x, eps, u, 5, 3, want_masks=True, flags=cd.sched_flags,
                    row0=row0, inputs=_inputs(cd, name, tau), want_ws=True)


def compare_step(name, tau, st, rtol=1e-4):
    d, p32, flat, x, eps, u = TR.setup(name)
    B = x.shape[0]
    what = f"{name} tau={tau} {'straight-through' if st else 'relaxed'}"
    gs, tail, masks, ws, cd = ystep(name, tau, st)
    Cc, g = _ref(name, tau, st)
    if st:
        assert Cc["gap"].min() > TR.MIN_GAP
    tail_gates(what, tail, B, Cc, rtol)
    check_grads(what, GM, d, gs, g, B, masks, Cc["pre"],
                lambda m: TR.loss_and_grads(d, p32, x, eps, u, tau, straight_through=st, weights=TR.case_weights(name),
                                            relu_masks=m)[1], rtol)
    return ws, cd, Cc


# (a) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", [False, True], ids=["relaxed", "straight_through"])
@pytest.mark.parametrize("tau", TR.TAUS)
@pytest.mark.parametrize("name", list(TR.CASES))
def test_step_matches_fp64_statement(name, tau, st):
    """Slot 0 holds tau, dims->temperature the decoy 1.0: a kernel that ignores the slot fails.  The weights case runs with
    GMVAE_OBJ_WEIGHTS (y_head_bwd_w's form)."""
    L = _L()
    ws, cd, Cc = compare_step(name, tau, st)
    want = "general" + ("+weights" if TR.case_weights(name) else "") + "+temp" + ("+st" if st else "")
    assert L.step_schedule(cd, GM) == want
    if st:                                    # the workspace's y: exact one-hot rows at the statement's argmax
        d, B = TR.CASES[name][0], TR.CASES[name][1]
        off = L.workspace_offset(cd, GM, "y") // 4
        y = ws[off:off + B * d.S * d.K].view(B * d.S, d.K).cpu().numpy()
        assert np.array_equal(y, Cc["y"])


# (b), (f) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.7, 0.1])
def test_slot_temperature_gives_the_bits_of_the_step_without_the_bit(tau):
    """K = 65 (the three-pass head): GMVAE_Y_TEMP_DEV with slot tau against the step without the bit at dims->temperature =
    tau, on the general schedule both: the tail and every gradient, bit for bit."""
    L = _L()
    name = "K65-S2"
    g0, t0, _, _, cd0 = ystep(name, tau, False, temp_dev=False)
    assert L.step_schedule(cd0, GM) == "general"
    g1, t1, _, _, cd1 = ystep(name, tau, False, temp_dev=True, temperature=1.0)
    assert L.step_schedule(cd1, GM) == "general+temp"
    assert np.isfinite(g0).all() and np.isfinite(t0).all()
    assert np.array_equal(g0, g1) and np.array_equal(t0, t1)


@pytest.mark.parametrize("name", ["K7-S3", "K17"])
def test_slot_temperature_identity_in_the_other_k_regimes(name):
    """The same identity where the step without the bit can be held to the general schedule by its sizes alone (hidden layers
    or samples the one-launch steps do not take) -- K <= 16 with a ragged last wave -- and, for K = 17, under the library's
    own switches."""
    import os
    L = _L()
    env = {"GMVAE_NO_MEGA": "1", "GMVAE_NO_SKINNY": "1", "GMVAE_NO_FUSED": "1"} if name == "K17" else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        g0, t0, _, _, cd0 = ystep(name, 0.7, False, temp_dev=False)
        assert L.step_schedule(cd0, GM) == "general"
        g1, t1, _, _, _ = ystep(name, 0.7, False, temp_dev=True)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert np.isfinite(g0).all() and np.isfinite(t0).all() and np.array_equal(g0, g1) and np.array_equal(t0, t1)


@pytest.mark.parametrize("name", list(TR.CASES))
def test_low_temperature_straight_through(name):
    """tau = 0.1 under straight-through at the project's 1e-4 (the gate the parent's relaxed errors select: module docstring)."""
    compare_step(name, 0.1, True)


# (c) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TR.CASES))
def test_forward_under_straight_through(name):
    import torch
    L = _L()
    tau = 0.5
    d, p32, flat, x, eps, u = TR.setup(name)
    B, R, K = x.shape[0], x.shape[0] * d.S, d.K
    cd = _cdims(name, B, True, True, 1.0)
    params, xd, ed, ud = dev(flat, torch.float32), dev(x, torch.uint8), dev(eps, torch.float32), dev(u, torch.float32)
    ws = torch.zeros(L.workspace_bytes(cd, GM) // 4 + 64, dtype=torch.float32, device="cuda")
    write_inputs(ws, cd, GM, _inputs(cd, name, tau))
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    tail, rows, z, y, lg = nan(L.TAIL), nan(R, 4), nan(R, d.L), nan(R, K), nan(B, K)
    L.check(L.lib.gmvae_forward(C.byref(cd), GM, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail), L.ptr(rows),
                                L.ptr(z), L.ptr(y), L.ptr(lg), L.ptr(ws), 5, 3, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    Cc, _ = _ref(name, tau, True)
    assert np.array_equal(y.cpu().numpy(), Cc["y"])                      # exact one-hot rows at the statement's argmax
    off = L.workspace_offset(cd, GM, "y_soft") // 4
    ys = ws[off:off + R * K].view(R, K).cpu().numpy().astype(np.float64)
    assert np.abs(ys.sum(axis=1) - 1.0).max() <= 1e-6
    assert np.abs(ys - Cc["y_soft"]).max() <= 1e-5
    _, ts, _, _, _ = ystep(name, tau, True)
    assert np.array_equal(tail[:5].cpu().numpy().astype(np.float64), ts[:5])      # the step's tail, bit for bit
    assert np.abs(lg.cpu().numpy() - Cc["logits"]).max() <= 1e-4 * max(np.abs(Cc["logits"]).max(), 1.0)


# (d) ------------------------------------------------------------------------------------------------------------
def _engine(seed, y_estimator, **kw):
    from gmvae_amd.engine import Engine
    d = TR.CASES["K7-weights"][0]
    return Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=seed, temperature=1.5, temperature_on_device=True,
                  y_estimator=y_estimator, **kw)


ROWS = ((2.0, 1.0, 0.5), (0.75, 0.3, 4.0))


def _eager(a, xs, rows):
    tails = []
    for t, tau in enumerate(rows):
        a.set_temperature(tau)
        tails.append(a.train_step(xs[t], lr=LR).clone())
    return tails


@pytest.mark.parametrize("y_estimator", ["relaxed", "straight_through"])
def test_train_graph_reads_one_temperature_per_step(y_estimator):
    """A 3-step train graph with temperatures (2.0, 1.0, 0.5) ends on the parameter bits of three eager steps that
    set_temperature to them; a second replay with new values matches again."""
    import torch
    d, B = TR.CASES["K7-weights"][0], 16
    xs = torch.from_numpy((np.random.default_rng(8).random((6, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(11, y_estimator), _engine(11, y_estimator)
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=3)
    assert replay.y_temperature.shape == (3,)
    assert torch.equal(replay.y_temperature.cpu(), torch.tensor([1.5] * 3))          # pre-filled: the engine's temperature
    for r, rows in enumerate(ROWS):
        tails = _eager(a, xs[3 * r:3 * r + 3], rows)
        sx.copy_(xs[3 * r:3 * r + 3])
        replay.y_temperature.copy_(torch.tensor(rows, dtype=torch.float32))
        replay()
        torch.cuda.synchronize()
        assert a.global_step == b.global_step == 3 * (r + 1)
        for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
            assert torch.equal(u.detach(), v.detach())
        assert torch.equal(replay.tail_log, torch.stack(tails)) and torch.isfinite(replay.tail_log).all()
    assert a.temperature == 4.0 and a.dims(B).temperature == 4.0 and b.temperature == 1.5
    with pytest.raises(ValueError):
        b.capture_train_step(B, lr=LR, n_steps=_L().LABEL_SLOTS + 1)
    with pytest.raises(ValueError, match="capture_train_step"):
        b.capture_train_pipeline(None, B, lr=LR, n_steps=2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            b.set_temperature(bad)


def test_dp_graph_with_a_one_rank_communicator():
    import torch
    need_rccl()
    L = _L()
    d, B = TR.CASES["K7-weights"][0], 16
    xs = torch.from_numpy((np.random.default_rng(10).random((6, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(13, "straight_through"), _engine(13, "straight_through")
    b.enable_rccl()
    try:
        sb, rb = b.capture_train_step(B, lr=LR, all_reduce=True, n_steps=3)
        assert b.dp_mode == "rccl-in-hipgraph"
        for r, rows in enumerate(ROWS):
            tails = _eager(a, xs[3 * r:3 * r + 3], rows)
            sb.copy_(xs[3 * r:3 * r + 3])
            rb.y_temperature.copy_(torch.tensor(rows, dtype=torch.float32))
            rb()
            torch.cuda.synchronize()
            for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
                assert torch.equal(u.detach(), v.detach())
            assert torch.equal(rb.tail_log, torch.stack(tails))
        a.set_temperature(0.6)
        b.set_temperature(0.6)
        t_a = a.train_step(xs[0], lr=LR).clone()
        t_b = b.dp_step(xs[0], LR).clone()
        torch.cuda.synchronize()
        assert torch.equal(t_a, t_b) and torch.equal(a.params.detach(), b.params.detach())
    finally:
        drop_comm(b)


# (e) ------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """n_steps = 33, the pipeline graph, the marginal bits and the VAE family: the error code, and a NaN-filled gradient buffer
    stays NaN everywhere."""
    import torch
    L = _L()
    name = "K7-weights"
    d, p32, flat, x, eps, u = TR.setup(name)
    B = x.shape[0]
    d1 = dataclasses.replace(d, temperature=1.0)
    xd, params = dev(x, torch.uint8), dev(flat, torch.float32)
    P = flat.size
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    m, v = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    step_dev = torch.zeros(2, dtype=torch.int64, device="cuda")
    for bits in (L.Y_TEMP_DEV, L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH):
        cd = dims_of(d1, B)
        cd.sched_flags = bits
        ws = torch.zeros(L.workspace_bytes(cd, GM) // 4 + 64, dtype=torch.float32, device="cuda")
        off = L.workspace_offset(cd, GM, "y_temperature") // 4
        ws[off:off + L.LABEL_SLOTS].fill_(1.0)
        xs = torch.zeros(33, B, d.D, dtype=torch.uint8, device="cuda")
        h = C.c_void_p()
        assert L.lib.gmvae_train_graph_create(C.byref(cd), GM, L.ptr(xs), 33, L.ptr(params), L.ptr(m), L.ptr(v), L.ptr(grads),
                                              L.ptr(ws), 0, L.ptr(step_dev), LR, 0.9, 0.999, 1e-8, None, C.byref(h)) == -2
        idx = torch.zeros(2, B, dtype=torch.int32, device="cuda")
        pix = torch.zeros(64, d.D, dtype=torch.uint8, device="cuda")
        assert L.lib.gmvae_train_graph_create_pipeline(C.byref(cd), GM, L.ptr(pix), 64, L.ptr(idx), L.ptr(xs), 2, L.ptr(params),
                                                       L.ptr(m), L.ptr(v), L.ptr(grads), L.ptr(ws), 0, L.ptr(step_dev), LR, 0.9,
                                                       0.999, 1e-8, None, C.byref(h)) == -2
        tail = torch.full((L.TAIL,), float("nan"), device="cuda")
        for extra in (L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW):
            cm = dims_of(d1, B)
            cm.sched_flags = bits | extra
            assert L.lib.gmvae_step(C.byref(cm), GM, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                                    L.current_stream()) == -2
            assert L.lib.gmvae_forward(C.byref(cm), GM, L.ptr(xd), None, None, L.ptr(params), L.ptr(tail), None, None, None,
                                       None, L.ptr(ws), 0, 0, L.current_stream()) == -2
        for model in (O.MODEL_VAE, O.MODEL_VAE_GMP):
            assert L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                                    L.current_stream()) == -3
            assert L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(tail), None, None, None,
                                       None, L.ptr(ws), 0, 0, L.current_stream()) == -3
        torch.cuda.synchronize()
        assert torch.isnan(grads).all() and torch.isnan(tail).all()                 # nothing was launched


# (g) ------------------------------------------------------------------------------------------------------------
def test_runner_anneals_and_continues_after_a_restore(tmp_path):
    """run_train with an annealed temperature takes the non-pipeline graph branch, places temperature_at of the true step
    indices in the graph's temperatures, and a second run restored from the first's checkpoint continues the schedule."""
    import torch
    from gmvae_amd import run_gmvae, runners
    base = ["--model=gmvae", f"--logdir={tmp_path}/run", "--random_seed=3", "--synthetic_size=512", "--batch_size=16",
            "--temperature=2", "--temperature_min=0.5", "--temperature_anneal_rate=0.2", "--temperature_anneal_every=2",
            "--y_estimator=straight_through", "--mode=train", "--summarise_every=4"]
    p = run_gmvae.build_parser()
    log = []

    def run(max_steps):
        cfg = run_gmvae.check_args(p, p.parse_args(base + [f"--max_steps={max_steps}"]))
        cfg.fault_hook = lambda eng: log.append((list(runners.run_train.temperature_log),
                                                 [r.y_temperature.cpu().tolist() for k, (_, r, _) in eng._graphs.items()
                                                  if getattr(r, "y_temperature", None) is not None and len(r.y_temperature) == len(runners.run_train.temperature_log)]))
        m = runners.run_train(cfg)
        assert runners.run_train.last_path == "graph+temp"
        return cfg, m

    cfg, m = run(7)
    e = m._engine
    assert e.temperature_on_device and e.y_estimator == "straight_through" and e.global_step == 8
    cfg, m2 = run(11)                                       # restored at step 8: the schedule continues there
    assert m2._engine.global_step == 12
    seen = [t for placed, _ in log for t, _ in placed]
    assert seen == list(range(12)), seen
    for placed, on_device in log:
        for t, tau in placed:
            assert tau == runners.temperature_at(cfg, t), (t, tau)
        assert on_device and on_device[0] == [float(np.float32(tau)) for _, tau in placed]
    taus = [tau for placed, _ in log for _, tau in placed]
    assert taus[0] == taus[1] == 2.0 and taus[2] == 2.0 * math.exp(-0.2 * 2 * 1) and taus[6] == 2.0 * math.exp(-0.2 * 2 * 3) and taus[8] == taus[9] == 0.5
    assert taus[-1] == 0.5
    assert torch.isfinite(m2._engine.params).all()
