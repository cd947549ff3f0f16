"""The GMVAE objective with y summed out exactly over its K values (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y, csrc/ymarg.hpp) on
the device: the step against the fp64 statement (tests/ymarg_ref.py) at the gates of hip_util.compare_step, the in-kernel
noise against gmvae_noise_fill, row shards against the whole batch, the forward outputs, train graphs (eager vs captured,
pipeline, data parallel with a one-rank communicator), an 8-step trajectory, the error codes and the runner end to end."""
import ctypes as C
import dataclasses
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import ymarg_ref as YM
from hip_util import _L, check_grads, dev, dims_of, drop_comm, hip_step, tail_gates

pytestmark = pytest.mark.gpu

LR = 1e-3
SIZES = {       # name: (Dims, B)
    "run_gmvae_defaults": (O.Dims(D=784, L=8, K=10, hidden=(64,)), 16),
    "configs2": (O.Dims(D=784, L=64, K=10, hidden=(64,)), 1024),
    "run_train_sh": (O.Dims(D=784, L=128, K=10, hidden=(512,)), 64),
    "k1": (O.Dims(D=784, L=8, K=1, hidden=(64,)), 32),
    "k64": (O.Dims(D=784, L=32, K=64, hidden=(64,)), 128),
    "h64x64_tanh": (O.Dims(D=200, L=16, K=7, hidden=(64, 64), act="tanh"), 24),
    "h24x2_relu": (O.Dims(D=100, L=5, K=7, hidden=(24, 24)), 8),
    "bias_vec": (O.Dims(D=784, L=8, K=10, hidden=(64,), gen_bias_init=np.linspace(-2.0, 1.0, 784)), 16),
}


def _mdims(d, B, row0=0):
    cd = dims_of(dataclasses.replace(d, S=1), B)
    cd.sched_flags = _L().OBJ_MARGINAL_Y
    cd.row0 = row0
    return cd


def _setup(d, B, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.05, p[k].shape)
    flat = O.pack(O.MODEL_GMVAE, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * d.K, d.L)).astype(np.float32)
    return flat, x, eps


def mstep(d, flat, x, eps, row0=0, seed=5, step=3):
    """One marginal gmvae_step: (grad sums [P] float64, tail [8], the step's ReLU masks)."""
    return hip_step(O.MODEL_GMVAE, dataclasses.replace(d, S=1), flat, x, eps, None, seed, step, want_masks=True,
                    flags=_L().OBJ_MARGINAL_Y, row0=row0, mask_rows=d.K)


def compare_step(d, flat, x, eps, what, row0=0, grad_rtol=1e-4, ref=None):
    """ref: the statement's (C, g) on these arguments where the caller holds it already."""
    B = x.shape[0]
    p32 = O.unpack(O.MODEL_GMVAE, d, flat.astype(np.float64))
    gs, tail, masks = mstep(d, flat, x, eps, row0=row0)
    Cc, g = ref or YM.loss_and_grads(d, p32, x, eps)
    tail_gates(what, tail, B, Cc)
    check_grads(what, O.MODEL_GMVAE, d, gs, g, B, masks, Cc["pre"], lambda m: YM.loss_and_grads(d, p32, x, eps, relu_masks=m)[1],
                grad_rtol)
    return gs, tail, Cc


@pytest.mark.parametrize("name", list(SIZES))
def test_step_matches_fp64_statement(name):
    d, B = SIZES[name]
    flat, x, eps = _setup(d, B, seed=len(name))
    compare_step(d, flat, x, eps, name)


def test_row0_and_in_kernel_noise_is_noise_fill():
    """eps = NULL draws gmvae_noise_fill's rows (row_base = row0 * K): the same bits as feeding those rows; row0 != 0."""
    import torch
    L = _L()
    d, B = SIZES["run_gmvae_defaults"]
    flat, x, _ = _setup(d, B, seed=3)
    row0, seed, step = 48, 5, 3
    g0, t0, _ = mstep(d, flat, x, None, row0=row0, seed=seed, step=step)
    eps = torch.zeros(B * d.K, d.L, dtype=torch.float32, device="cuda")
    L.check(L.lib.gmvae_noise_fill(L.ptr(eps), None, B * d.K, d.L, d.K, row0 * d.K, seed, step, None, L.current_stream()),
            "gmvae_noise_fill")
    torch.cuda.synchronize()
    e = eps.cpu().numpy()
    g1, t1, _ = mstep(d, flat, x, e, row0=row0, seed=seed, step=step)
    assert np.array_equal(g0, g1) and np.array_equal(t0, t1)
    compare_step(d, flat, x, e, "row0", row0=row0)


def test_row_shards_add_up_to_the_batch():
    d, _ = SIZES["run_gmvae_defaults"]
    B = 64
    flat, x, _ = _setup(d, B, seed=4)
    gf, tf, _ = mstep(d, flat, x, None)
    ga, ta, _ = mstep(d, flat, x[:B // 2], None, row0=0)
    gb, tb, _ = mstep(d, flat, x[B // 2:], None, row0=B // 2)
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        n = int(np.prod(shape))
        ref = gf[off:off + n]
        assert np.abs(ga[off:off + n] + gb[off:off + n] - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-6), name
    np.testing.assert_allclose(ta[:4] + tb[:4], tf[:4], rtol=1e-5)
    assert ta[4] + tb[4] == tf[4] == B


def test_forward_outputs():
    import torch
    L = _L()
    d, B = SIZES["run_gmvae_defaults"]
    flat, x, eps = _setup(d, B, seed=6)
    R = B * d.K
    cd = _mdims(d, B)
    params, xd, ed = dev(flat, torch.float32), dev(x, torch.uint8), dev(eps, torch.float32)
    f32 = dict(dtype=torch.float32, device="cuda")
    tail, rows, z = torch.zeros(L.TAIL, **f32), torch.zeros(R, 4, **f32), torch.zeros(R, d.L, **f32)
    y, lg = torch.zeros(R, d.K, **f32), torch.zeros(B, d.K, **f32)
    ws = torch.zeros(L.workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, **f32)
    L.check(L.lib.gmvae_forward(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), L.ptr(ed), None, L.ptr(params), L.ptr(tail), L.ptr(rows),
                                L.ptr(z), L.ptr(y), L.ptr(lg), L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    tail, rows, z, y, lg = (t.cpu().numpy().astype(np.float64) for t in (tail, rows, z, y, lg))
    _, ts, Cc = compare_step(d, flat, x, eps, "forward")
    np.testing.assert_allclose(tail[:5], ts[:5], rtol=1e-6)
    tail_gates("forward", tail, B, Cc)
    np.testing.assert_allclose(rows, Cc["rows"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(z, Cc["z"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(lg, Cc["logits"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(y, np.tile(np.eye(d.K), (B, 1)))


def _engine(d, seed, **kw):
    from gmvae_amd.engine import Engine
    return Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=seed, y_inference="marginal", **kw)


def test_engine_api():
    import torch
    from gmvae_amd import gmvae
    d, B = SIZES["run_gmvae_defaults"]
    e = _engine(d, 1)
    x = torch.from_numpy(_setup(d, B)[1]).cuda()
    o = e.forward(x)
    assert o["rows"].shape == (B * d.K, 4) and o["z"].shape == (B * d.K, d.L) and o["y"].shape == (B * d.K, d.K)
    assert o["logits"].shape == (B, d.K)
    with pytest.raises(ValueError):
        e.step(x, u=torch.rand(B, d.K))
    with pytest.raises(ValueError):
        e.step(x, eps=torch.zeros(B, d.L))              # eps has B*K rows
    with pytest.raises(ValueError, match="marginal"):
        e.iw_bound(x, 10)
    loss = e.loss(x, torch.zeros(B * d.K, d.L))
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(e.params.grad).all()
    # a checkpoint of either mode loads in the other
    m = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=2,
                           y_inference="marginal")
    g = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=3)
    g.load_state_dict(m.state_dict())
    assert torch.equal(g.params, m.params)


def test_error_codes():
    import torch
    L = _L()
    d, B = SIZES["run_gmvae_defaults"]
    flat, x, _ = _setup(d, B)
    xd, params = dev(x, torch.uint8), dev(flat, torch.float32)
    grads = torch.zeros(flat.size + L.TAIL, device="cuda")
    ws = torch.zeros(1 << 22, device="cuda")
    for model in (O.MODEL_VAE, O.MODEL_VAE_GMP):
        cd = _mdims(d, B)
        assert L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                                L.current_stream()) == -3
    cd = _mdims(d, B)
    cd.S = 2
    assert L.lib.gmvae_step(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                            L.current_stream()) == -2
    tail = torch.zeros(L.TAIL, device="cuda")
    assert L.lib.gmvae_iw_bound(C.byref(_mdims(d, B)), O.MODEL_GMVAE, L.ptr(xd), L.ptr(params), 10, None, None, L.ptr(tail),
                                L.ptr(ws), 0, 0, L.current_stream()) == -2
    assert L.step_schedule(_mdims(d, B), O.MODEL_GMVAE) == "general+marginal"
    assert L.step_schedule(L.make_dims(1024, 784, 64, 10, (64,)), O.MODEL_GMVAE) == "mega2"


def test_train_graph_is_eager_steps_bit_for_bit():
    import torch
    d, B = SIZES["run_gmvae_defaults"]
    xs = torch.from_numpy((np.random.default_rng(8).random((4, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(d, 11), _engine(d, 11)
    for t in range(4):
        a.train_step(xs[t], lr=LR)
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=4)
    sx.copy_(xs)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 4
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    # the per-step tails of the graph are the eager steps' tails (the last one checked here)
    assert torch.equal(replay.tail_log[3], a.grads[a.P:])


def test_pipeline_graph_is_binarise_then_step():
    import torch
    from gmvae_amd.data import DeviceDataset, binarize
    from gmvae_amd.engine import Engine
    d, B = SIZES["run_gmvae_defaults"]
    n = 3
    pix = np.random.default_rng(9).integers(0, 256, (300, d.D), dtype=np.uint8)
    a, b = _engine(d, 12), _engine(d, 12)
    replay = a.capture_train_pipeline(DeviceDataset(pix, shuffle=True, seed=21), B, lr=LR, n_steps=n)
    replay()
    torch.cuda.synchronize()
    ds = DeviceDataset(pix, shuffle=True, seed=21)
    for step in range(n):
        rows = ds.next_rows(B)
        x = binarize(ds.pixels, rows=rows, seed=b.noise_seed ^ Engine.BINARIZE_SEED_XOR, step=step)
        assert torch.equal(x, replay.batches[step]) and torch.equal(rows, replay.rows[step])
        b.train_step(x, lr=LR)
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == n
    assert torch.equal(a.params.detach(), b.params.detach())


def test_dp_graph_one_rank_is_the_single_device_graph():
    import torch
    d, B = SIZES["run_gmvae_defaults"]
    xs = torch.from_numpy((np.random.default_rng(10).random((2, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(d, 13), _engine(d, 13)
    b.enable_rccl()
    try:
        sa, ra = a.capture_train_step(B, lr=LR, n_steps=2)
        sb, rb = b.capture_train_step(B, lr=LR, all_reduce=True, n_steps=2)
        assert b.dp_mode == "rccl-in-hipgraph"
        sa.copy_(xs)
        sb.copy_(xs)
        ra()
        rb()
        b.dp_step(xs[0], LR)
        a.train_step(xs[0], lr=LR)
        torch.cuda.synchronize()
        assert torch.equal(a.params.detach(), b.params.detach()) and torch.equal(a.v, b.v)
    finally:
        drop_comm(b)


def test_trajectory_follows_fp64_statement():
    """8 eager train steps on injected noise against 8 fp64 statement steps + oracle.adam_tf_step (fp64).  Every step's loss
    terms at the step gates against fp64 at the device's own parameters; the trajectory's parameter updates agree to 2 %
    (Adam normalises every coordinate: where a gradient is within rounding of zero its step's sign is arbitrary)."""
    import torch
    d, B = SIZES["h24x2_relu"]
    n = 8
    e = _engine(d, 14)
    flat0 = e.params.detach().cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(15)
    xs = (rng.random((n, B, d.D)) < 0.87).astype(np.uint8)
    epss = rng.standard_normal((n, B * d.K, d.L)).astype(np.float32)
    ref = flat0.copy()
    m, v = np.zeros_like(ref), np.zeros_like(ref)
    for t in range(n):
        pre = e.params.detach().cpu().numpy().astype(np.float64)
        tail = e.train_step(torch.from_numpy(xs[t]).cuda(), eps=torch.from_numpy(epss[t]).cuda(), lr=LR).cpu().numpy()
        Cd, _ = YM.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, pre), xs[t], epss[t])
        tail_gates(f"step {t}", tail.astype(np.float64), B, Cd)
        _, g = YM.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, ref), xs[t], epss[t])
        ref, m, v = O.adam_tf_step(ref, m, v, O.pack(O.MODEL_GMVAE, d, g, np.float64), t + 1, lr=LR, dtype=np.float64)
    fin = e.params.detach().cpu().numpy().astype(np.float64)
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        k = int(np.prod(shape))
        dd, dr = fin[off:off + k] - flat0[off:off + k], ref[off:off + k] - flat0[off:off + k]
        assert np.linalg.norm(dd - dr) <= 0.02 * max(np.linalg.norm(dr), 1e-12), name


def test_runner_trains_and_evaluates(tmp_path):
    logdir = str(tmp_path / "run")
    common = [sys.executable, "-m", "gmvae_amd.run_gmvae", f"--logdir={logdir}", "--y_inference=marginal", "--random_seed=3",
              "--synthetic_size=2048", "--batch_size=64"]
    r = subprocess.run(common + ["--mode=train", "--max_steps=300", "--summarise_every=50"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import glob
    import os
    import re
    assert glob.glob(os.path.join(logdir, "*")), "no checkpoint written"
    losses = [float(v) for v in re.findall(r"loss[^0-9\-]*(-?[0-9.]+(?:e[-+]?\d+)?)", r.stdout + r.stderr)]
    assert len(losses) >= 2 and all(np.isfinite(losses)) and losses[-1] < losses[0], (r.stdout[-2000:], r.stderr[-2000:])
    r = subprocess.run(common + ["--mode=eval", "--checkpoint_max_wait=5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for key in ("loss_per_example", "nll", "kl_div_z", "nent"):
        assert re.search(rf"train/{key}: (-?[0-9.]+)", r.stdout), (key, r.stdout[-2000:])
