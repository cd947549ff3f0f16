"""The semi-supervised GMVAE objective (include/gmvae_hip.h GMVAE_OBJ_LABELS, csrc/semisup.hpp ymarg_sup_rows / sup_tail) on the
device: the step against the fp64 statement (tests/semisup_ref.py) at the gates of tests/test_ymarg_iw.py, with DReG, a batch
without labels against the step without the bit bit for bit, alpha = 0, row shards, the forward outputs, train graphs with one
label set per step (single device and a one-rank communicator) against eager steps bit for bit, the refusals, an 8-step
trajectory, a learning test and the runner end to end."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import oracle as O
import semisup_ref as SR
from hip_util import _L, check_grads, dev, dims_of, drop_comm, hip_step, tail_gates, workspace, write_inputs

pytestmark = pytest.mark.gpu

LR = 1e-3
ALPHA = 0.7
CASES = {       # name: (Dims, B, S)
    "a": (O.Dims(D=200, L=8, K=10, hidden=(64,)), 6, 1),                         # B no multiple of the 4 waves of a workgroup
    "b": (O.Dims(D=200, L=8, K=10, hidden=(64,)), 6, 3),
    "c": (O.Dims(D=200, L=8, K=80, hidden=(64,)), 5, 2),                         # a label >= 64: the lane loop's second pass
    "d": (O.Dims(D=100, L=5, K=3, hidden=(24,)), 8, 70),                         # S > 64
    "e": (O.Dims(D=200, L=16, K=7, hidden=(64, 64), act="tanh"), 9, 2),
}
SEEDS = {"a": 1, "b": 2, "c": 3, "d": 4, "e": 5}      # every labelled example's two largest q differ by > 1e-3 in fp64 (asserted)
TOP2_GAP = 1e-3


def _labels(K, B, seed):
    """Roughly half -1, half uniform in [0, K); always 0 and K - 1, and one out-of-range value (K) that must behave as -1."""
    rng = np.random.default_rng(1000 + seed)
    y = np.where(rng.random(B) < 0.5, -1, rng.integers(0, K, B)).astype(np.int32)
    y[0], y[1], y[2], y[-1] = 0, K - 1, K, -1
    return y


def _setup(d, B, S, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.05, p[k].shape)
    flat = O.pack(O.MODEL_GMVAE, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * S * d.K, d.L)).astype(np.float32)
    return flat, x, eps


def _sdims(d, B, S, row0=0, flags=None):
    L = _L()
    cd = dims_of(dataclasses.replace(d, S=S), B)
    cd.sched_flags = (L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS) if flags is None else flags
    cd.row0 = row0
    return cd


def _workspace(cd, y, alpha):
    """A zeroed workspace with the caller's two regions filled: every label set -1, set 0 = y, the classification weight."""
    ws = workspace(cd, O.MODEL_GMVAE)
    if cd.sched_flags & _L().OBJ_LABELS:
        write_inputs(ws, cd, O.MODEL_GMVAE, {"labels": y, "sup_weight": alpha})
    return ws


def sstep(d, S, flat, x, eps, y, alpha, row0=0, seed=5, step=3, flags=None):
    """One gmvae_step with the bit: (grad sums [P] float64, tail [8], the step's ReLU masks)."""
    L = _L()
    flags = (L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS) if flags is None else flags
    return hip_step(O.MODEL_GMVAE, dataclasses.replace(d, S=S), flat, x, eps, None, seed, step, want_masks=True, flags=flags,
                    row0=row0, mask_rows=S * d.K, inputs={"labels": y, "sup_weight": alpha} if flags & L.OBJ_LABELS else None)


def _terms_ok(tail, B, Cc, what, hits=True):
    print(f"{what}: ref ce {Cc['ce']} n {Cc['n_labelled']} hits {Cc['hits']}")
    tail_gates(what, tail, B, Cc)
    assert abs(tail[5] - Cc["ce"]) <= 1e-4 * max(abs(Cc["ce"]), 1.0), (what, tail[5], Cc["ce"])
    assert tail[6] == Cc["n_labelled"] and (tail[7] == Cc["hits"] or not hits), (what, tail[6:], Cc["n_labelled"], Cc["hits"])


def compare_step(d, S, flat, x, eps, y, alpha, what, flags=None, estimator="standard", grad_rtol=1e-4, ref=None):
    """ref: the statement's (C, g) on these arguments where the caller holds it already."""
    B = x.shape[0]
    p32 = O.unpack(O.MODEL_GMVAE, d, flat.astype(np.float64))
    gs, tail, masks = sstep(d, S, flat, x, eps, y, alpha, flags=flags)
    Cc, g = ref or SR.loss_and_grads(d, p32, x, eps, S, y, alpha, estimator=estimator)
    gap = Cc["top2_gap"][Cc["labelled"]]
    assert gap.size == 0 or gap.min() > TOP2_GAP, (what, gap.min())      # hits is unambiguous at fp32
    _terms_ok(tail, B, Cc, what)
    check_grads(what, O.MODEL_GMVAE, d, gs, g, B, masks, Cc["pre"],
                lambda m: SR.loss_and_grads(d, p32, x, eps, S, y, alpha, relu_masks=m, estimator=estimator)[1], grad_rtol)
    return gs, tail, Cc


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_step_matches_fp64_statement(name):
    d, B, S = CASES[name]
    flat, x, eps = _setup(d, B, S, seed=SEEDS[name])
    y = _labels(d.K, B, SEEDS[name])
    if name == "c":
        y[3] = 71                                   # a label in the second pass of the lane loop
    assert (y == 0).any() and (y == d.K - 1).any() and (y == d.K).any() and (y == -1).any()
    _, tail, Cc = compare_step(d, S, flat, x, eps, y, ALPHA, name)
    assert Cc["n_labelled"] == int(((y >= 0) & (y < d.K)).sum()) >= 2


# 2 --------------------------------------------------------------------------------------------------------------
def test_step_with_dreg_matches_fp64_statement():
    L = _L()
    d, B, S = CASES["b"]
    flat, x, eps = _setup(d, B, S, seed=SEEDS["b"])
    compare_step(d, S, flat, x, eps, _labels(d.K, B, SEEDS["b"]), ALPHA, "b+dreg",
                 flags=L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS | L.GRAD_DREG, estimator="dreg")


# 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
def test_no_labels_is_the_step_without_the_bit_bit_for_bit(S):
    L = _L()
    d, B = CASES["a"][0], 6
    flat, x, eps = _setup(d, B, S, seed=2)
    y = np.full(B, -1, np.int32)
    objs = [L.OBJ_MARGINAL_Y_IW] + ([L.OBJ_MARGINAL_Y] if S == 1 else [])
    for obj in objs:
        for e in (eps, None):
            g1, t1, _ = sstep(d, S, flat, x, e, y, 0.37, flags=obj | L.OBJ_LABELS)
            g0, t0, _ = sstep(d, S, flat, x, e, y, 0.0, flags=obj)
            assert np.array_equal(g1, g0) and np.array_equal(t1[:5], t0[:5]), (obj, e is None)
            assert not t1[5:].any() and not t0[5:].any()


# 4 --------------------------------------------------------------------------------------------------------------
def test_all_labelled_without_classification_weight_leaves_encoder_y_alone():
    d, B, S = CASES["b"]
    flat, x, eps = _setup(d, B, S, seed=SEEDS["b"])
    y = np.random.default_rng(4).integers(0, d.K, B).astype(np.int32)
    gs, tail, Cc = compare_step(d, S, flat, x, eps, y, 0.0, "alpha0")
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        if name.startswith("encoder_y_fcnet/"):
            assert not gs[off:off + int(np.prod(shape))].any(), name
    assert tail[3] == 0 and tail[6] == B


# 5 --------------------------------------------------------------------------------------------------------------
def test_row_shards_add_up():
    d, S, B = CASES["a"][0], 2, 12
    flat, x, _ = _setup(d, B, S, seed=6)
    y = _labels(d.K, B, 6)
    gf, tf, _ = sstep(d, S, flat, x, None, y, ALPHA)
    ga, ta, _ = sstep(d, S, flat, x[:B // 2], None, y[:B // 2], ALPHA, row0=0)
    gb, tb, _ = sstep(d, S, flat, x[B // 2:], None, y[B // 2:], ALPHA, row0=B // 2)
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        n = int(np.prod(shape))
        ref = gf[off:off + n]
        assert np.abs(ga[off:off + n] + gb[off:off + n] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-6), name
    np.testing.assert_allclose(ta[:8] + tb[:8], tf[:8], rtol=1e-5)
    assert ta[6] + tb[6] == tf[6] == int(((y >= 0) & (y < d.K)).sum()) and ta[7] + tb[7] == tf[7]


# 6 --------------------------------------------------------------------------------------------------------------
def test_forward_outputs():
    import torch
    L = _L()
    d, B, S = CASES["b"]
    flat, x, eps = _setup(d, B, S, seed=SEEDS["b"])
    y = _labels(d.K, B, SEEDS["b"])
    R = B * S * d.K
    cd = _sdims(d, B, S)
    params, xd, ed = dev(flat, torch.float32), dev(x, torch.uint8), dev(eps, torch.float32)
    f32 = dict(dtype=torch.float32, device="cuda")
    tail, rows, z = torch.zeros(L.TAIL, **f32), torch.zeros(R, 4, **f32), torch.zeros(R, d.L, **f32)
    yo, lg = torch.zeros(R, d.K, **f32), torch.zeros(B, d.K, **f32)
    ws = _workspace(cd, y, ALPHA)
    L.check(L.lib.gmvae_forward(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), L.ptr(ed), None, L.ptr(params), L.ptr(tail), L.ptr(rows),
                                L.ptr(z), L.ptr(yo), L.ptr(lg), L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    tail, rows, z, yo, lg = (t.cpu().numpy().astype(np.float64) for t in (tail, rows, z, yo, lg))
    _, ts, Cc = compare_step(d, S, flat, x, eps, y, ALPHA, "forward")
    assert np.array_equal(tail, ts)
    np.testing.assert_allclose(rows, Cc["rows"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(z, Cc["z"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(lg, Cc["logits"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(yo, np.tile(np.eye(d.K), (B * S, 1)))


# 7 --------------------------------------------------------------------------------------------------------------
def _engine(d, seed, y_inference="marginal_iw", **kw):
    from gmvae_amd.engine import Engine
    return Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=seed, y_inference=y_inference, **kw)


def _three_label_sets(K, B):
    import torch
    ys = np.stack([_labels(K, B, 20 + t) for t in range(3)])
    ys[1] = -1                                                                   # one step of the graph without labels
    ys[2] = np.random.default_rng(5).integers(0, K, B)                           # one all labelled
    return torch.from_numpy(ys).cuda()


def test_train_graph_reads_one_label_set_per_step():
    import torch
    d, B = CASES["a"][0], 16
    xs = torch.from_numpy((np.random.default_rng(8).random((3, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    ys = _three_label_sets(d.K, B)
    kw = dict(n_samples=2, semi_supervised=True, sup_weight=ALPHA)
    a, b = _engine(d, 11, **kw), _engine(d, 11, **kw)
    tails = []
    for t in range(3):
        tails.append(a.train_step(xs[t], lr=LR, y_observed=ys[t]).clone())
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=3)
    assert replay.y_observed.shape == (3, B) and replay.y_observed.dtype == torch.int32 and (replay.y_observed == -1).all()
    sx.copy_(xs)
    replay.y_observed.copy_(ys)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 3
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log, torch.stack(tails))
    n_lab = ((ys >= 0) & (ys < d.K)).sum(dim=1).float()
    assert torch.equal(replay.tail_log[:, 6].cpu(), n_lab.cpu()) and replay.tail_log[1, 5:].abs().sum().item() == 0
    with pytest.raises(ValueError):
        b.capture_train_step(B, lr=LR, n_steps=_L().LABEL_SLOTS + 1)
    with pytest.raises(ValueError):
        _engine(d, 11, n_samples=2).step(xs[0], y_observed=ys[0])                # y_observed needs the option


def test_dp_graph_one_rank_reads_one_label_set_per_step():
    import torch
    d, B = CASES["a"][0], 16
    xs = torch.from_numpy((np.random.default_rng(10).random((3, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    ys = _three_label_sets(d.K, B)
    kw = dict(n_samples=2, semi_supervised=True, sup_weight=ALPHA)
    a, b = _engine(d, 13, **kw), _engine(d, 13, **kw)
    b.enable_rccl()
    try:
        tails = [a.train_step(xs[t], lr=LR, y_observed=ys[t]).clone() for t in range(3)]
        sb, rb = b.capture_train_step(B, lr=LR, all_reduce=True, n_steps=3)
        assert b.dp_mode == "rccl-in-hipgraph"
        sb.copy_(xs)
        rb.y_observed.copy_(ys)
        rb()
        tails.append(a.train_step(xs[0], lr=LR, y_observed=ys[2]).clone())
        t4 = b.dp_step(xs[0], LR, y_observed=ys[2]).clone()
        torch.cuda.synchronize()
        for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
            assert torch.equal(u.detach(), v.detach())
        assert torch.equal(rb.tail_log, torch.stack(tails[:3])) and torch.equal(t4, tails[3])
    finally:
        drop_comm(b)


# 8 --------------------------------------------------------------------------------------------------------------
def test_device_side_refusals():
    import torch
    from gmvae_amd.data import DeviceDataset
    L = _L()
    d, B, S = CASES["a"][0], 16, 2
    flat, x, _ = _setup(d, B, S)
    xd, params = dev(x, torch.uint8), dev(flat, torch.float32)
    P = flat.size
    grads, m, v = torch.zeros(P + L.TAIL, device="cuda"), torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    step_dev = torch.zeros(2, dtype=torch.int64, device="cuda")
    cd = _sdims(d, B, S)
    ws = _workspace(cd, np.full(B, -1), 1.0)
    xs = torch.zeros(33, B, d.D, dtype=torch.uint8, device="cuda")
    h = C.c_void_p()
    assert L.lib.gmvae_train_graph_create(C.byref(cd), O.MODEL_GMVAE, L.ptr(xs), 33, L.ptr(params), L.ptr(m), L.ptr(v),
                                          L.ptr(grads), L.ptr(ws), 0, L.ptr(step_dev), LR, 0.9, 0.999, 1e-8, None, C.byref(h)) == -2
    idx = torch.zeros(2, B, dtype=torch.int32, device="cuda")
    pix = torch.zeros(64, d.D, dtype=torch.uint8, device="cuda")
    assert L.lib.gmvae_train_graph_create_pipeline(C.byref(cd), O.MODEL_GMVAE, L.ptr(pix), 64, L.ptr(idx), L.ptr(xs), 2,
                                                   L.ptr(params), L.ptr(m), L.ptr(v), L.ptr(grads), L.ptr(ws), 0, L.ptr(step_dev),
                                                   LR, 0.9, 0.999, 1e-8, None, C.byref(h)) == -2
    gumbel = _sdims(d, B, S, flags=L.OBJ_LABELS)
    assert L.lib.gmvae_step(C.byref(gumbel), O.MODEL_GMVAE, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0,
                            None, L.current_stream()) == -2
    for model in (O.MODEL_VAE, O.MODEL_VAE_GMP):
        assert L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                                L.current_stream()) == -3
    torch.cuda.synchronize()
    assert not grads.any()                                                      # nothing was launched
    e = _engine(d, 1, n_samples=2, semi_supervised=True)
    with pytest.raises(ValueError, match="label gather"):
        e.capture_train_pipeline(DeviceDataset(np.zeros((64, d.D), np.uint8), shuffle=False), B)


# 9 --------------------------------------------------------------------------------------------------------------
def test_trajectory_follows_fp64_statement():
    """8 eager train steps on injected noise against 8 fp64 statement steps + oracle.adam_tf_step (fp64), at the gates of
    tests/test_ymarg_iw.py::test_trajectory_follows_fp64_statement."""
    import torch
    d, B, S = CASES["a"][0], 16, 1
    n = 8
    e = _engine(d, 14, n_samples=S, semi_supervised=True, sup_weight=ALPHA)
    flat0 = e.params.detach().cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(15)
    xs = (rng.random((n, B, d.D)) < 0.87).astype(np.uint8)
    epss = rng.standard_normal((n, B * S * d.K, d.L)).astype(np.float32)
    ys = np.stack([_labels(d.K, B, 30 + t) for t in range(n)])
    ref = flat0.copy()
    m, v = np.zeros_like(ref), np.zeros_like(ref)
    for t in range(n):
        pre = e.params.detach().cpu().numpy().astype(np.float64)
        tail = e.train_step(torch.from_numpy(xs[t]).cuda(), eps=torch.from_numpy(epss[t]).cuda(), lr=LR,
                            y_observed=torch.from_numpy(ys[t]).cuda()).cpu().numpy().astype(np.float64)
        Cd, _ = SR.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, pre), xs[t], epss[t], S, ys[t], ALPHA)
        # (hits is compared where no labelled example's two largest q are within TOP2_GAP at the device's own parameters)
        _terms_ok(tail, B, Cd, f"step {t}", hits=Cd["top2_gap"][Cd["labelled"]].min() > TOP2_GAP)
        _, g = SR.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, ref), xs[t], epss[t], S, ys[t], ALPHA)
        ref, m, v = O.adam_tf_step(ref, m, v, O.pack(O.MODEL_GMVAE, d, g, np.float64), t + 1, lr=LR, dtype=np.float64)
    fin = e.params.detach().cpu().numpy().astype(np.float64)
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        k = int(np.prod(shape))
        dd, dr = fin[off:off + k] - flat0[off:off + k], ref[off:off + k] - flat0[off:off + k]
        assert np.linalg.norm(dd - dr) <= 0.02 * max(np.linalg.norm(dr), 1e-12), name


# 10 -------------------------------------------------------------------------------------------------------------
PROTO_SEED = 0      # the fp64 statement (fp64_learning below, its own N(0,1) draws) ends at hits / n_labelled = 1.0 with this seed
LEARN = dict(D=64, H=32, L=4, K=4, B=32, steps=200, lr=1e-2, flip=0.05)


def _learning_batches(seed):
    """Four fixed random prototypes, one per class; every example is its class's prototype with each pixel flipped with
    probability 0.05.  (x [steps, B, D] uint8, y [steps, B] int32)."""
    c = LEARN
    rng = np.random.default_rng(seed)
    protos = (rng.random((c["K"], c["D"])) < 0.5).astype(np.uint8)
    y = rng.integers(0, c["K"], (c["steps"], c["B"])).astype(np.int32)
    flips = rng.random((c["steps"], c["B"], c["D"])) < c["flip"]
    return protos[y] ^ flips.astype(np.uint8), y


def fp64_learning(seed):
    """The same 200 steps through the fp64 statement and the oracle's TF-Adam: the final step's hits / n_labelled."""
    c = LEARN
    d = O.Dims(D=c["D"], L=c["L"], K=c["K"], hidden=(c["H"],))
    xs, ys = _learning_batches(seed)
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    ref = O.pack(O.MODEL_GMVAE, d, p, np.float64)
    m, v = np.zeros_like(ref), np.zeros_like(ref)
    rng = np.random.default_rng(seed + 1)
    for t in range(c["steps"]):
        eps = rng.standard_normal((c["B"] * c["K"], c["L"]))
        Cc, g = SR.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, ref), xs[t], eps, 1, ys[t], 1.0)
        ref, m, v = O.adam_tf_step(ref, m, v, O.pack(O.MODEL_GMVAE, d, g, np.float64), t + 1, lr=c["lr"], dtype=np.float64)
    return Cc["hits"] / Cc["n_labelled"]


def test_labels_teach_the_classifier():
    """All labelled, alpha = 1: after 200 steps q(y|x) names the observed component.  A behavioural floor (0.9; the fp64
    statement reaches >= 0.98 at this prototype seed, the room covers the different noise draws), not a parity gate."""
    import torch
    c = LEARN
    d = O.Dims(D=c["D"], L=c["L"], K=c["K"], hidden=(c["H"],))
    xs, ys = _learning_batches(PROTO_SEED)
    e = _engine(d, 3, y_inference="marginal", semi_supervised=True, sup_weight=1.0)
    xd, yd = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()
    for t in range(c["steps"]):
        tail = e.train_step(xd[t], lr=c["lr"], y_observed=yd[t])
    tail = tail.cpu().numpy()
    print(f"learning: final tail {tail.tolist()}")
    assert tail[6] == c["B"] and np.isfinite(tail).all()
    assert tail[7] / tail[6] >= 0.9, tail


# 11 -------------------------------------------------------------------------------------------------------------
def test_runner_end_to_end(tmp_path, capsys):
    import re
    import torch
    from gmvae_amd import gmvae, run_gmvae, runners
    common = ["--model=gmvae", "--y_inference=marginal", "--labelled_per_class", "20", f"--logdir={tmp_path}/run",
              "--random_seed=3", "--synthetic_size=2048", "--batch_size=64"]
    m = run_gmvae.main(common + ["--mode=train", "--max_steps", "20", "--summarise_every", "10"])
    out = capsys.readouterr().out
    assert runners.run_train.last_path == "graph+labels"
    assert m._engine.semi_supervised and m._engine.global_step == 21
    assert re.search(r"sup_acc [0-9.]+  sup_ce [0-9.]+", out), out[-2000:]
    run_gmvae.main(common + ["--mode=eval", "--checkpoint_max_wait=5"])
    out = capsys.readouterr().out
    acc = re.search(r"train/class_acc_q: ([0-9.e+\-]+)", out)
    assert acc and 0.0 <= float(acc.group(1)) <= 1.0, out[-2000:]
    # the parameters are the same with and without the option: the checkpoint loads into a plain engine
    g = gmvae.create_gmvae(784, 8, mixture_components=10, fcnet_hidden_sizes=[64], random_seed=9, y_inference="marginal")
    g.load_state_dict(torch.load(runners._ckpt(run_gmvae.build_parser().parse_args(common)), map_location="cpu"))
    assert not g._engine.semi_supervised and torch.equal(g.params.detach(), m.params.detach())
