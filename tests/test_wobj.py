"""The weighted objective (GMVAE_OBJ_WEIGHTS) on the device: the step through the C ABI on explicit noise against the fp64
statement (tests/wobj_ref.py) at the project's gates -- loss at 1e-4 relative, nll / kl / nent each relative to itself, every
gradient tensor at 1e-4 of its own max, tail[5..7] exact -- then the graph, data-parallel, runner and model-API paths."""
import numpy as np
import pytest

import oracle as O
import wobj_ref as WR
from hip_util import _L, check_grads, dims_of, drop_comm, grad_errs, hip_step, need_rccl, tail_gates

pytestmark = pytest.mark.gpu

LR = 1e-3
_REF = {}          # (case, weights) -> the fp64 statement's (C, g): computed once, shared, left unchanged


def _ref(name, weights):
    key = (name, tuple(weights))
    if key not in _REF:
        model, marginal, d, p32, flat, x, eps, u = WR.setup(name)
        _REF[key] = WR.loss_and_grads(model, d, p32, x, eps, u, weights, marginal)
    return _REF[key]


def _cdims(model, marginal, d, B, bit=True):
    L = _L()
    cd = dims_of(d, B)
    cd.sched_flags = (L.OBJ_MARGINAL_Y if marginal else 0) | (L.OBJ_WEIGHTS if bit else 0)
    return cd


def wstep(model, marginal, d, flat, x, eps, u, weights, bit=True, row0=0):
    """One gmvae_step at row0 (slot 0 of the weight rows = weights): (grad sums [P] float64, tail [8], the step's ReLU masks)."""
    return hip_step(model, d, flat, x, eps, u, 5, 3, want_masks=True, flags=_cdims(model, marginal, d, x.shape[0], bit).sched_flags,
                    row0=row0, mask_rows=d.K if marginal else 1, inputs={"obj_weights": list(weights) + [0.0]} if bit else None)


def compare_step(name, weights, what, case=None, ref=None):
    """case, ref: parameters and inputs in WR.setup's form and their statement (C, g), where they are not the case's own Xavier
    ones (tests/test_objectives_saturated.py)."""
    model, marginal, d, p32, flat, x, eps, u = case or WR.setup(name)
    B = x.shape[0]
    gs, tail, masks = wstep(model, marginal, d, flat, x, eps, u, weights)
    Cc, g = ref or _ref(name, weights)
    tail_gates(what, tail, B, Cc)
    w32 = np.asarray(weights, np.float32)
    assert tail[5] == float(np.float32(B) * w32[0]) and tail[6] == float(np.float32(B) * w32[1]), (what, tail[5:7])
    assert tail[7] == Cc["floor"].sum(), (what, tail[7], Cc["floor"])
    check_grads(what, model, d, gs, g, B, masks, Cc["pre"],
                lambda m: WR.loss_and_grads(model, d, p32, x, eps, u, weights, marginal, relu_masks=m)[1])
    return gs, tail


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WR.CASES))
def test_step_matches_fp64_statement(name):
    """Weights (0.25, 2.0, lambda), lambda the midpoint of the widest gap of the statement's own sorted KL_y (two values more
    than 1e-3 nat apart, examples on both sides: asserted here and, without a device, in tests/test_wobj_cpu.py)."""
    mname, marginal, d, B = WR.CASES[name]
    lam = WR.case_lambda(name)
    weights = WR.WEIGHTS + (lam,)
    if mname == "gmvae":
        C0, _ = _ref(name, (1.0, 1.0, 0.0))
        assert np.abs(C0["kl_y"] - lam).min() > 5e-4 and (C0["kl_y"] < lam).any() and (C0["kl_y"] > lam).any()
    if name.endswith("one-launch-sizes"):
        L = _L()
        model = O.MODEL_NAMES[mname]
        assert L.step_schedule(_cdims(model, marginal, d, B, bit=False), model) != "general" or marginal
        assert L.step_schedule(_cdims(model, marginal, d, B), model) == ("general+marginal+weights" if marginal else "general+weights")
    compare_step(name, weights, name)


# 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "vae_gmp", "gumbel", "marginal", "gumbel-one-launch-sizes"])
def test_unit_weights_match_the_step_without_the_bit(name):
    """Weights (1, 1, 0) against the step without the bit, at the same gates (not bit for bit: the fp64 sum forming l_bk is
    ordered differently, and the one-launch step sums in its own order)."""
    model, marginal, d, p32, flat, x, eps, u = WR.setup(name)
    B = x.shape[0]
    gw, tw, _ = wstep(model, marginal, d, flat, x, eps, u, (1.0, 1.0, 0.0))
    g0, t0, _ = wstep(model, marginal, d, flat, x, eps, u, None, bit=False)
    print(f"{name}: with the bit {tw.tolist()} without {t0.tolist()}")
    assert abs(tw[0] - t0[0]) <= 1e-4 * abs(t0[0])
    assert abs(tw[1] - t0[1]) <= 1e-4 * abs(t0[1])
    assert abs(tw[2] - t0[2]) <= 1e-4 * max(abs(t0[2]), B) and abs(tw[3] - t0[3]) <= 1e-4 * max(abs(t0[3]), B)
    assert tw[4] == t0[4] == B and tw[5] == B and tw[6] == B and tw[7] == 0 and (t0[5:] == 0).all()
    lay, _, _ = O.param_layout(model, d)
    for pname, shape, off in lay:
        n = int(np.prod(shape))
        a, b = gw[off:off + n], g0[off:off + n]
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-6 * B)
        print(f"{name} {pname}: rel-to-max diff {err:.3e}")
        assert err <= 1e-4, (pname, err)


# 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gumbel", "marginal"])
def test_uniform_logits_without_floor(name):
    """lambda = 0 with exactly uniform logits (the y encoder's output layer zeroed: nent_b = -ln K up to rounding, the edge at
    which a comparison against 0 - ln K could fall either way): the loss is finite and no example sits on a floor."""
    model, marginal, d, p32, flat, x, eps, u = WR.setup(name)
    lay, _, _ = O.param_layout(model, d)
    flat = flat.copy()
    nl = len(d.hidden)
    for pname, shape, off in lay:
        if pname in (f"encoder_y_fcnet/linear_{nl}/w", f"encoder_y_fcnet/linear_{nl}/b"):
            flat[off:off + int(np.prod(shape))] = 0.0
    gs, tail, _ = wstep(model, marginal, d, flat, x, eps, u, (0.25, 2.0, 0.0))
    print(f"{name}: tail {tail.tolist()}")
    assert np.isfinite(tail).all() and np.isfinite(gs).all()
    assert tail[7] == 0
    assert abs(tail[3] / x.shape[0] + np.log(d.K)) <= 1e-5


# 4 --------------------------------------------------------------------------------------------------------------
def _engine(name, seed, **kw):
    from gmvae_amd.engine import Engine
    mname, marginal, d, B = WR.CASES[name]
    return Engine(mname, d.D, d.L, d.K, list(d.hidden), random_seed=seed, temperature=d.temperature, sigma_min=d.sigma_min,
                  y_inference="marginal" if marginal else "gumbel", weighted_objective=True, **kw)


ROWS8 = [(0.125 * (i + 1), 0.25 * (i + 1), 0.0 if i % 3 == 0 else 0.05 * i) for i in range(8)]


@pytest.mark.parametrize("name", ["gumbel", "marginal", "vae_gmp"])
def test_train_graph_reads_one_weight_row_per_step(name):
    """An 8-step train graph with eight different weight rows ends on the parameter bits of eight eager steps that
    set_objective_weights to those rows."""
    import torch
    d, B = WR.CASES[name][2], 16
    xs = torch.from_numpy((np.random.default_rng(8).random((8, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(name, 11, kl_weight=0.5, y_weight=0.75, y_free_nats=0.1), _engine(name, 11, kl_weight=0.5, y_weight=0.75, y_free_nats=0.1)
    tails = []
    for t in range(8):
        a.set_objective_weights(*ROWS8[t])
        tails.append(a.train_step(xs[t], lr=LR).clone())
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=8)
    assert replay.obj_weights.shape == (8, 4)
    assert torch.equal(replay.obj_weights.cpu(), torch.tensor([[0.5, 0.75, 0.1, 0.0]] * 8))      # pre-filled: the engine's weights
    sx.copy_(xs)
    replay.obj_weights.copy_(torch.tensor([r + (0.0,) for r in ROWS8], dtype=torch.float32))
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 8
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log, torch.stack(tails))
    want = torch.tensor([r[0] for r in ROWS8], dtype=torch.float32) * B
    assert torch.equal(replay.tail_log[:, 5].cpu(), want)
    with pytest.raises(ValueError):
        b.capture_train_step(B, lr=LR, n_steps=_L().LABEL_SLOTS + 1)
    with pytest.raises(ValueError, match="capture_train_step"):
        b.capture_train_pipeline(None, B, lr=LR, n_steps=2)


# 5 --------------------------------------------------------------------------------------------------------------
def test_dp_step_and_dp_graph_with_a_one_rank_communicator():
    import torch
    need_rccl()
    name = "marginal"
    d, B = WR.CASES[name][2], 16
    xs = torch.from_numpy((np.random.default_rng(10).random((2, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(name, 13), _engine(name, 13)
    b.enable_rccl()
    try:
        tails = []
        for t in range(2):
            a.set_objective_weights(*ROWS8[t + 1])
            tails.append(a.train_step(xs[t], lr=LR).clone())
        sb, rb = b.capture_train_step(B, lr=LR, all_reduce=True, n_steps=2)
        assert b.dp_mode == "rccl-in-hipgraph"
        sb.copy_(xs)
        rb.obj_weights.copy_(torch.tensor([ROWS8[1] + (0.0,), ROWS8[2] + (0.0,)], dtype=torch.float32))
        rb()
        a.set_objective_weights(*ROWS8[5])
        b.set_objective_weights(*ROWS8[5])
        tails.append(a.train_step(xs[0], lr=LR).clone())
        t3 = b.dp_step(xs[0], LR).clone()
        torch.cuda.synchronize()
        for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
            assert torch.equal(u.detach(), v.detach())
        assert torch.equal(rb.tail_log, torch.stack(tails[:2])) and torch.equal(t3, tails[2])
        assert t3[5].item() == B * np.float32(ROWS8[5][0])
    finally:
        drop_comm(b)


# (the eager fallback of a refused data-parallel graph: tests/test_step_inputs.py, for all four per-step inputs)


# 6 --------------------------------------------------------------------------------------------------------------
def test_runner_follows_the_warmup_schedule(tmp_path):
    """run_train for 12 steps on synthetic pixels with --kl_warmup_steps 8: the logged tail[5] / tail[4] is the schedule, exactly
    (batch 16: the division by B is exact), through capture_train_step."""
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", f"--logdir={tmp_path}/run", "--random_seed=3", "--synthetic_size=512", "--batch_size=16",
            "--kl_weight=0.5", "--y_weight=2", "--y_free_nats=0.05", "--kl_warmup_steps=8", "--mode=train", "--max_steps=11",
            "--summarise_every=4"]
    p = run_gmvae.build_parser()
    cfg = run_gmvae.check_args(p, p.parse_args(args))
    log = []                                                 # (run_train keeps the last summary block's steps: collected per block)
    cfg.fault_hook = lambda eng: log.extend(runners.run_train.weight_log)
    m = runners.run_train(cfg)
    assert runners.run_train.last_path == "graph+weights"
    assert m._engine.weighted_objective and m._engine.global_step == 12
    assert [s for s, _, _ in runners.run_train.weight_log] == [9, 10, 11, 12]
    assert [s for s, _, _ in log] == list(range(1, 13))
    for step, kw, yw in log:
        f = runners.kl_warmup(step - 1, 8)
        assert kw == float(np.float32(0.5 * f)) and yw == float(np.float32(2.0 * f)), (step, kw, yw)
    assert log[0][1] == 0.0625 and log[7][1] == log[11][1] == 0.5


# 7 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gumbel", "marginal", "vae_gmp"])
def test_model_api_matches_fp64_statement(name):
    """create_gmvae / create_vae(weighted_objective=...): run_model followed by backward() against the statement; the summaries
    keep nll / kl / nent unweighted and add the weights and the floor's share."""
    import torch
    import torch.nn.functional as F
    from gmvae_amd import gmvae, vae
    mname, marginal, d, B = WR.CASES[name]
    model, _, _, p32, flat, x, eps, u = WR.setup(name)
    lam = WR.case_lambda(name)
    weights = WR.WEIGHTS + (lam,)
    kw = dict(fcnet_hidden_sizes=list(d.hidden), sigma_min=d.sigma_min, raw_sigma_bias=d.raw_sigma_bias, random_seed=1,
              weighted_objective=True, kl_weight=weights[0], y_weight=weights[1], y_free_nats=weights[2])
    if mname == "gmvae":
        m = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, temperature=d.temperature,
                               y_inference="marginal" if marginal else "gumbel", **kw)
    else:
        m = vae.create_vae(d.D, d.L, mixture_components=d.K, **kw)
    e = m._engine
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(flat).cuda())
    xt = torch.from_numpy(x).cuda()
    et = torch.from_numpy(eps).cuda()
    if mname == "gmvae":
        loss = m.run_model(xt, xt, eps=et, u=None if marginal else torch.from_numpy(u).cuda())
    else:
        loss = m.run_model(xt, xt, eps=et)
    loss.backward()
    torch.cuda.synchronize()
    Cc, g = _ref(name, weights)
    assert abs(loss.item() - Cc["loss"]) <= 1e-4 * abs(Cc["loss"])
    s = {k: v.item() for k, v in m.summaries.items() if k != "cluster_acc"}
    print(f"{name}: summaries {s}")
    assert abs(s["nll_scalar"] - Cc["nll"]) <= 1e-4 * abs(Cc["nll"]) and abs(s["kl_div_z"] - Cc["kl"]) <= 1e-4 * max(abs(Cc["kl"]), 1.0)
    assert s["kl_weight"] == float(np.float32(weights[0])) and s["y_weight"] == float(np.float32(weights[1]))
    assert s["y_floor_share"] == Cc["floor"].mean()
    gs = e.params.grad.detach().cpu().numpy().astype(np.float64) * B
    for pname, err in grad_errs(model, d, gs, g, B):
        print(f"{name} {pname}: rel-to-max err {err:.3e}")
        assert err <= 1e-4, (pname, err)
