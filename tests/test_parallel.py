"""world_size-2 gloo tests (CPU) of the data-parallel plumbing: row sharding, the single flat
all-reduce with the loss sums and count in the tail, and the replicated TF-Adam update.  The
per-rank compute is the oracle (no GPU here); the -m gpu twin below runs the HIP step on one GPU
split into two 'ranks' in-process."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle as O
from gmvae_amd import parallel as par


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _local_buffer(model, d, flat, x, eps, u):
    """What gmvae_step leaves in the flat buffer: gradient SUMS + [loss, nll, kl, nent, count] sums."""
    B = x.shape[0]
    C, g = O.loss_and_grads(model, d, O.unpack(model, d, flat), x, eps, u, np.float64)
    P = flat.size
    buf = np.zeros(P + par.TAIL)
    buf[:P] = O.pack(model, d, g, np.float64) * B
    buf[P:P + 5] = [C["loss"] * B, C["nll"] * B, C["kl"] * B, C["nent"] * B, B]
    return buf


def _worker(rank, world, port, Bg, steps, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    r, w, _ = par.init_from_env("gloo")
    assert (r, w) == (rank, world)
    model, d = O.MODEL_GMVAE, O.Dims(D=40, L=4, K=3, hidden=(8,))
    flat = O.pack(model, d, O.init_params(model, d, np.random.default_rng(0)), np.float64)
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    P = flat.size
    losses = []
    for t in range(1, steps + 1):
        x, eps, u = O.make_inputs(d, Bg, seed_x=t, seed_noise=100 + t)
        a, b = par.shard_rows(Bg, rank, world)
        buf = torch.from_numpy(_local_buffer(model, d, flat, x[a:b], eps[a:b], u[a:b]))
        par.all_reduce_flat(buf)                       # the ONE collective of the step
        scale = par.grad_scale(buf, P).item()
        assert buf[P + 4].item() == Bg
        flat, m, v = O.adam_tf_step(flat, m, v, buf[:P].numpy() * scale, t, dtype=np.float64)
        losses.append(buf[P].item() * scale)
    assert par.assert_replicas_identical(torch.from_numpy(flat))
    out[rank] = (flat, losses)
    dist.destroy_process_group()


@pytest.mark.parametrize("Bg", [16, 15])            # 15: uneven shards (8 + 7 rows)
def test_two_rank_gloo_equals_single_process(Bg):
    steps, world = 3, 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), Bg, steps, out), nprocs=world, join=True)
    model, d = O.MODEL_GMVAE, O.Dims(D=40, L=4, K=3, hidden=(8,))
    flat = O.pack(model, d, O.init_params(model, d, np.random.default_rng(0)), np.float64)
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    ref_losses = []
    for t in range(1, steps + 1):
        x, eps, u = O.make_inputs(d, Bg, seed_x=t, seed_noise=100 + t)
        flat, m, v, C, _ = O.train_step(model, d, flat, m, v, t, x, eps, u, dtype=np.float64)
        ref_losses.append(C["loss"])
    f0, l0 = out[0]
    f1, l1 = out[1]
    assert np.array_equal(f0, f1)                                   # replicas bit-identical
    np.testing.assert_allclose(l0, ref_losses, rtol=1e-12)
    # Adam divides by sqrt(v)+eps: reduction-order noise (1e-16) on near-dead coordinates is amplified
    np.testing.assert_allclose(f0, flat, rtol=0, atol=1e-9)


def _default_seed_worker(rank, world, port, Bg, steps, out):
    """What `torchrun ... run_gmvae` with the reference's default --random_seed=None does on every rank: parameters and
    noise seed drawn from this PROCESS's entropy, then broadcast_state from rank 0, then data-parallel steps whose
    noise rows are keyed by the GLOBAL row (rank's shard start + local row), as the HIP step keys its Philox counters."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    par.init_from_env("gloo")
    model, d = O.MODEL_GMVAE, O.Dims(D=40, L=6, K=3, hidden=(8,))
    own = np.random.default_rng()                                   # entropy: different on every rank
    flat_t = torch.from_numpy(O.pack(model, d, O.init_params(model, d, own), np.float64))
    m_t, v_t = torch.zeros_like(flat_t), torch.zeros_like(flat_t)
    seed0 = int(own.integers(1, 2 ** 62))
    start = flat_t.clone()
    seed, gstep = par.broadcast_state((flat_t, m_t, v_t), (seed0, 0))
    if rank != 0:
        assert not torch.equal(start, flat_t) and seed != seed0     # the ranks really started apart
    flat, m, v = flat_t.numpy().copy(), m_t.numpy(), v_t.numpy()
    P = flat.size
    for t in range(1, steps + 1):
        x = (np.random.default_rng(t).random((Bg, d.D)) < 0.87).astype(np.uint8)
        a, b = par.shard_rows(Bg, rank, world)
        eps, u = O.noise(b - a, d.L, d.K, a, seed, gstep + t - 1)   # rows a .. b-1 of the global stream
        buf = torch.from_numpy(_local_buffer(model, d, flat, x[a:b], eps, u))
        par.all_reduce_flat(buf)
        flat, m, v = O.adam_tf_step(flat, m, v, buf[:P].numpy() * par.grad_scale(buf, P).item(), t, dtype=np.float64)
    assert par.assert_replicas_identical(torch.from_numpy(flat))
    out[rank] = (flat, seed, flat_t.numpy().copy())
    dist.destroy_process_group()


def test_default_seeded_ranks_are_synchronised_and_draw_the_global_noise_rows():
    """ADVICE r1 (high) + VERDICT r1 items 2-3: (i) with random_seed=None the ranks end bit-identical because the
    start state is broadcast; (ii) the 2-rank run equals ONE process stepping the global batch with the global noise
    stream (same eps/u rows), not two copies of one shard's noise."""
    steps, world, Bg = 3, 2, 14
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_default_seed_worker, args=(world, _free_port(), Bg, steps, out), nprocs=world, join=True)
    (f0, s0, init0), (f1, s1, init1) = out[0], out[1]
    assert s0 == s1 and np.array_equal(init0, init1) and np.array_equal(f0, f1)
    model, d = O.MODEL_GMVAE, O.Dims(D=40, L=6, K=3, hidden=(8,))
    flat, m, v = init0.copy(), np.zeros_like(init0), np.zeros_like(init0)
    for t in range(1, steps + 1):
        x = (np.random.default_rng(t).random((Bg, d.D)) < 0.87).astype(np.uint8)
        eps, u = O.noise(Bg, d.L, d.K, 0, s0, t - 1)
        flat, m, v, _, _ = O.train_step(model, d, flat, m, v, t, x, eps, u, dtype=np.float64)
    np.testing.assert_allclose(f0, flat, rtol=0, atol=1e-9)
    # and the shards' noise really differs (the round-1 defect: every rank drew rows 0 .. B/G-1)
    e0, _ = O.noise(7, d.L, d.K, 0, s0, 0)
    e1, _ = O.noise(7, d.L, d.K, 7, s0, 0)
    assert not np.array_equal(e0, e1)


def _hist_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    par.init_from_env("gloo")
    from gmvae_amd.utils import cluster_acc_from_hist
    rng = np.random.default_rng(5)
    logits, labels = rng.normal(size=(300, 10)), rng.integers(0, 10, 300)
    a, b = par.shard_rows(300, rank, world)
    hist = torch.zeros(10, 10, dtype=torch.int64)                      # what cluster_hist leaves on each rank
    hist.index_put_((torch.from_numpy(logits[a:b].argmax(1)), torch.from_numpy(labels[a:b])), torch.ones(b - a, dtype=torch.int64),
                    accumulate=True)
    dist.all_reduce(hist)                                              # the collective of utils.cluster_acc(all_reduce=True)
    out[rank] = float(cluster_acc_from_hist(hist))
    dist.destroy_process_group()


def test_two_rank_cluster_acc_is_the_global_batch_accuracy():
    """the data-parallel definition of cluster_acc -- sum the [K, n_labels] histograms over the
    ranks, then take each cluster's majority -- equals scripts/utils.py:173-191 on the unsharded batch."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_hist_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    rng = np.random.default_rng(5)
    logits, labels = rng.normal(size=(300, 10)), rng.integers(0, 10, 300)
    want = O.cluster_acc(logits, labels, 10)
    assert abs(out[0] - want) < 1e-6 and out[0] == out[1]


def test_shard_rows_cover_and_balance():
    for n in (1, 7, 16, 1000, 1023):
        for w in (1, 2, 3, 8):
            spans = [par.shard_rows(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


@pytest.mark.gpu
def test_hip_step_sharded_sum_equals_full_batch():
    """1-GPU stand-in for the N-GPU equality: gradient SUMS of two row shards add up to the full-batch
    buffer (what the all-reduce computes), to fp32 reduction-order tolerance.
    Every other objective family and uneven shards at row0 != 0: tests/test_shards.py."""
    import hip_util as H
    d = O.Dims(D=784, L=16, K=10, hidden=(64,))
    model = O.MODEL_GMVAE
    flat = O.pack(model, d, O.init_params(model, d, np.random.default_rng(1)), np.float32)
    x, eps, u = O.make_inputs(d, 256)
    full, tail = H.hip_step(model, d, flat, x, eps, u)
    acc, tacc = 0.0, 0.0
    for r in range(2):
        a, b = par.shard_rows(256, r, 2)
        g, t = H.hip_step(model, d, flat, x[a:b], eps[a:b], u[a:b])
        acc, tacc = acc + g, tacc + t
    assert tacc[4] == tail[4] == 256
    assert abs(tacc[0] - tail[0]) <= 1e-5 * abs(tail[0])
    assert np.abs(acc - full).max() <= 2e-5 * np.abs(full).max()


@pytest.mark.gpu
@pytest.mark.parametrize("model,Lz,K,Bg,G,Hd", [("gmvae", 64, 10, 1024, 2, 64), ("gmvae", 64, 10, 2048, 4, 64), ("gmvae", 16, 10, 250, 2, 64),
                                               ("vae_gmp", 64, 10, 512, 2, 64), ("gmvae", 6, 7, 96, 3, 64),
                                               ("gmvae", 128, 10, 128, 2, 512),      # bin/run_train.sh sizes: the skinny schedule
                                               ("gmvae", 32, 7, 100, 3, 128)])       # (ragged row tiles, three shards)
def test_virtual_ranks_with_row_offsets_sum_to_the_full_batch_philox_step(model, Lz, K, Bg, G, Hd):
    """In-kernel Philox noise (eps = u = NULL) under data parallelism: G 'virtual ranks' on one GPU, each stepping
    its row shard with GmvaeDims.row0 = its first global row, leave gradient sums that add up to the single-device
    step on the whole batch with row0 = 0 -- same seed, same step, same eps/u rows.
    Every other objective family and uneven shards at row0 != 0: tests/test_shards.py."""
    import ctypes as C
    import hip_util as H
    from gmvae_amd import _lib as L
    mid = O.MODEL_NAMES[model]
    d = O.Dims(D=784, L=Lz, K=K, hidden=(Hd,))
    flat = O.pack(mid, d, O.init_params(mid, d, np.random.default_rng(1)), np.float32)
    x = (np.random.default_rng(2).random((Bg, 784)) < 0.87).astype(np.uint8)
    params = H.dev(flat, torch.float32)
    lay, _, _ = O.param_layout(mid, d)
    real = np.zeros(flat.size + L.TAIL, bool)                  # (the alignment padding between tensors is not part of the contract)
    for _, shape, off in lay:
        real[off:off + int(np.prod(shape))] = True
    real[flat.size:] = True

    def run(xs, row0):
        cd = H.dims_of(d, xs.shape[0])
        cd.row0 = row0
        P, _ = L.param_count(cd, mid)
        grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
        ws = H.workspace(cd, mid)
        xd = H.dev(xs, torch.uint8)
        L.check(L.lib.gmvae_step(C.byref(cd), mid, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 99, 4, None,
                                 L.current_stream()), "gmvae_step")
        torch.cuda.synchronize()
        g = grads.cpu().numpy().astype(np.float64)
        assert np.isfinite(g[real]).all()
        return np.where(real, g, 0.0)

    full = run(x, 0)
    acc = 0.0
    for r in range(G):
        a, b = par.shard_rows(Bg, r, G)
        acc = acc + run(x[a:b], a)
    P = full.size - L.TAIL
    assert acc[P + 4] == full[P + 4] == Bg
    assert abs(acc[P] - full[P]) <= 2e-6 * abs(full[P])                 # same noise rows: only the summation order differs
    assert np.abs(acc[:P] - full[:P]).max() <= 2e-5 * np.abs(full[:P]).max()
    # the defect this replaces: without the offset both shards draw rows 0 .. B/G-1 and the loss is measurably different
    wrong = sum(run(x[slice(*par.shard_rows(Bg, r, G))], 0) for r in range(G))
    assert abs(wrong[P] - full[P]) > 1e-5 * abs(full[P])


@pytest.mark.gpu
def test_config5_full_shard_is_the_sum_of_its_row_shards():
    """BASELINE configs[4]'s per-GPU shard at FULL size (D = 3072, K = 64, hidden 512, S = 50, B = 512: 25,600 sample rows -- far past
    what the oracle finishes in seconds), through a property that does not depend on size: with in-kernel Philox noise keyed by the
    GLOBAL row, the step on 512 rows leaves the sum of the steps on its four 128-row shards (row0 = 0, 128, 256, 384) -- gradient
    sums, loss sum and row count -- although the two runs take different slab counts, tile grids and per-tensor pair scales; and
    the full-size step is bit-identical when repeated.  (The 128-row shard itself is compared with the oracle in
    tests/test_hip_parity.py::test_plane_gemms_at_config5_dims_under_natural_gating.)
    Every other objective family and uneven shards at row0 != 0: tests/test_shards.py."""
    import ctypes as C
    import hip_util as H
    from gmvae_amd import _lib as L
    mid = O.MODEL_GMVAE
    d = O.Dims(D=3072, L=64, K=64, hidden=(512,), S=50)
    Bg, G = 512, 4
    flat = O.pack(mid, d, O.init_params(mid, d, np.random.default_rng(1)), np.float32)
    x = (np.random.default_rng(2).random((Bg, 3072)) < 0.3).astype(np.uint8)
    params = H.dev(flat, torch.float32)
    lay, _, _ = O.param_layout(mid, d)
    real = np.zeros(flat.size + L.TAIL, bool)
    for _, shape, off in lay:
        real[off:off + int(np.prod(shape))] = True
    real[flat.size:] = True

    def run(xs, row0):
        cd = H.dims_of(d, xs.shape[0])
        cd.row0 = row0
        assert L.step_schedule(cd, mid) == "general+planes"
        P, _ = L.param_count(cd, mid)
        grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
        ws = H.workspace(cd, mid)
        xd = H.dev(xs, torch.uint8)
        L.check(L.lib.gmvae_step(C.byref(cd), mid, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 7, 3, None,
                                 L.current_stream()), "gmvae_step")
        torch.cuda.synchronize()
        g = grads.cpu().numpy().astype(np.float64)
        assert np.isfinite(g[real]).all()
        return np.where(real, g, 0.0)

    full = run(x, 0)
    assert np.array_equal(full, run(x, 0))
    acc = 0.0
    for r in range(G):
        acc = acc + run(x[128 * r:128 * (r + 1)], 128 * r)
    P = full.size - L.TAIL
    assert acc[P + 4] == full[P + 4] == Bg
    assert abs(acc[P] - full[P]) <= 2e-6 * abs(full[P])
    assert np.abs(acc[:P] - full[:P]).max() <= 2e-5 * np.abs(full[:P]).max()


@pytest.mark.gpu
def test_rccl_in_library_world1_matches_plain_step():
    """The C-side RCCL path (communicator of one rank on this GPU): gmvae_dp_step and the captured DP graph
    give the same trajectory as step + Adam without any collective."""
    from gmvae_amd.engine import Engine
    x, _, _ = O.make_inputs(O.Dims(D=784, L=16, K=10, hidden=(64,)), 128)
    xt = torch.from_numpy(x).cuda()
    ref = Engine("gmvae", 784, 16, 10, [64], random_seed=5)
    for _ in range(4):
        ref.train_step(xt, lr=1e-3)
    e = Engine("gmvae", 784, 16, 10, [64], random_seed=5)
    e.enable_rccl()
    e.dp_step(xt, 1e-3)
    e.dp_step(xt, 1e-3)
    sx, replay = e.capture_train_step(128, lr=1e-3, all_reduce=True)
    sx.copy_(xt)
    replay()
    replay()
    torch.cuda.synchronize()
    assert e.global_step == ref.global_step == 4
    assert torch.allclose(e.params.detach(), ref.params.detach(), atol=1e-6)
    assert int(e.step_dev[0].item()) == 4


@pytest.mark.gpu
def test_rccl_multi_step_graph_world1_tracks_eager_steps():
    """The data-parallel train graph with several steps per launch: from its second step on the first layer runs inside
    mega_fwd_bwd on weight images that the Adam launch AFTER the all-reduce scattered (adam_tf_img).  With a
    one-rank communicator the all-reduce is the identity, so the trajectory must track plain eager steps."""
    from gmvae_amd.engine import Engine
    rng = np.random.default_rng(12)
    n, B = 3, 1024
    xs = torch.from_numpy((rng.random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()
    ref = Engine("gmvae", 784, 64, 10, [64], random_seed=6)
    for r in range(2):
        for i in range(n):
            ref.train_step(xs[i], lr=1e-3)
    e = Engine("gmvae", 784, 64, 10, [64], random_seed=6)
    e.enable_rccl()
    sx, replay = e.capture_train_step(B, lr=1e-3, all_reduce=True, n_steps=n)
    assert e.dp_mode == "rccl-in-hipgraph" and tuple(sx.shape) == (n, B, 784)
    sx.copy_(xs)
    replay()
    replay()
    torch.cuda.synchronize()
    assert e.global_step == ref.global_step == 2 * n and int(e.step_dev[0].item()) == 2 * n
    assert e.handoff_timeouts() == 0 and torch.isfinite(e.params).all()
    assert (e.params - ref.params).abs().max().item() < 2e-5
    assert abs(e.grads[e.P].item() - ref.grads[ref.P].item()) < 1e-4 * abs(ref.grads[ref.P].item())


# ------------------------------------------------------------------------------------------------ world 2 on ONE GPU
def _spawn_ranks(tmp_path, argv, world=2, timeout=420):
    """`world` fresh child processes of tests/dp_child.py (gloo, all on cuda:0, no mutual waits inside a launch)."""
    import subprocess
    import sys
    port = _free_port()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(world):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE=str(world),
                   LOCAL_RANK="0", GMVAE_DIST_BACKEND="gloo", GMVAE_NO_FL="1", GMVAE_MEGA_Q="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "dp_child.py")] + [str(a) for a in argv],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()                                   # exactly the PIDs started here
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{o[-3000:]}"
    return [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), map_location="cpu") for r in range(world)], outs


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_product_path_equals_the_global_batch_trajectory(tmp_path, monkeypatch):
    """The data-parallel PRODUCT path with world = 2 on hardware: two fresh processes, default seeding
    (random_seed=None: different initial weights), Engine.sync_replicas() + train_step(all_reduce=True) on their row shards
    of the same global batches.  Replicas must end bit-identical, and equal (fp32 summation order) to ONE process stepping
    the whole global batch from the same start: the Philox counters hold the global row, so the noise is the same."""
    from gmvae_amd.engine import Engine
    n, B = 5, 512
    res, _ = _spawn_ranks(tmp_path, ["engine", tmp_path, n, B])
    a, b = res
    assert a["start"]["differed"] or b["start"]["differed"]              # the ranks did start from different draws
    assert torch.equal(a["start"]["params"], b["start"]["params"]) and a["start"]["noise_seed"] == b["start"]["noise_seed"]
    for k in ("params", "m", "v", "tails"):
        assert torch.equal(a[k], b[k]), f"replicas differ in {k}"
    assert a["global_step"] == b["global_step"] == n and a["timeouts"] == b["timeouts"] == 0
    assert float(a["tails"][-1, 4]) == 2 * B                              # the all-reduced count is the global batch
    # one process, the global batch
    monkeypatch.setenv("GMVAE_NO_FL", "1")
    monkeypatch.setenv("GMVAE_MEGA_Q", "1")
    e = Engine("gmvae", 784, 64, 10, [64], random_seed=0)
    with torch.no_grad():
        e.params.copy_(a["start"]["params"].cuda())
    e.noise_seed = a["start"]["noise_seed"]
    xs = (np.random.default_rng(77).random((n, 2 * B, 784)) < 0.87).astype(np.uint8)
    tails = [e.train_step(torch.from_numpy(xs[t]).cuda(), lr=1e-3).clone().cpu() for t in range(n)]
    tails = torch.stack(tails)
    torch.cuda.synchronize()
    rel = (tails[:, 0] - a["tails"][:, 0]).abs() / a["tails"][:, 0].abs()
    assert rel.max().item() < 5e-6, rel                                   # per-step loss sums of the global batch
    # n TF-Adam steps at lr = 1e-3; the two computations differ in summation order only, which Adam's m / sqrt(v) amplifies
    # on coordinates with near-zero gradients: a mean gate and a loose max gate (as tests/test_runner.py)
    diff = (e.params.detach().cpu() - a["params"]).abs()
    assert diff.mean().item() < 5e-6 and diff.max().item() < n * 1e-3 * 0.2, (diff.mean().item(), diff.max().item())


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_run_gmvae_train(tmp_path):
    """`run_gmvae --mode=train` with WORLD_SIZE = 2 (default flags' seeding: --random_seed unset): the start state is
    broadcast, every rank applies the same all-reduced gradient, the replicas stay bit-identical and the loss falls."""
    args = ["--mode=train", "--model=gmvae", "--latent_size=64", "--batch_size=512", "--max_steps=39", "--summarise_every=10",
            f"--logdir={tmp_path}/log", "--synthetic_size=4096"]
    res, outs = _spawn_ranks(tmp_path, ["runner", tmp_path] + args)
    a, b = res
    for k in ("params", "m", "v"):
        assert torch.equal(a[k], b[k]), f"replicas differ in {k}"
    assert a["global_step"] == b["global_step"] == 40 and a["path"] == "dp-graph" and a["timeouts"] == 0
    assert a["dp_mode"] == "torch.distributed"                            # (gloo: the all-reduce between two eager halves)
    assert torch.isfinite(a["params"]).all() and 0 < a["loss"] < 500      # from D ln 2 - ln K = 541
    assert os.path.exists(os.path.join(tmp_path, "log", "gmvae", "h64_n1_z64", "model.pt"))
    assert "Step 40" in outs[0]


@pytest.mark.gpu
def test_bench_world2_branch_on_one_gpu_prints_a_marked_line(tmp_path):
    """bench.py's `world > 1` branch executed for real: two fresh child ranks on the one GPU of the box,
    `torch.distributed` over gloo (RCCL refuses two ranks on one device), started before anything touches the GPU.  This is
    a FALLBACK path by bench.py's own definition, so the JSON line must be printed anyway -- n_gpus 2, replicas
    bit-identical, "fallback": true with the reason and config.all_reduce naming the path that was timed -- and, without
    --allow-fallback, the exit code must be non-zero AFTER the line is out."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        port = _free_port()
        procs = []
        for r in range(2):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r),
                       GMVAE_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
                                           "--batch", "512", "--safe-schedule", "--full", "--no-cpu-baseline", "--no-iwae-bound"] + extra,
                                          env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        outs = []
        try:
            for p in procs:
                outs.append(p.communicate(timeout=420))
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()                               # exactly the PIDs started here
        return procs, outs

    procs, outs = run(["--allow-fallback"])
    for r, (p, (so, se)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{se[-3000:]}"
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and not [l for l in outs[1][0].splitlines() if l.startswith("{")]      # rank 0 prints ONE line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 20 and j["config"]["global_batch"] == 1024 and j["value"] > 0
    assert j["config"]["replicas_identical"] is True and j["config"]["safe_schedule"] is True
    assert j["fallback"] is True and j["fallback_reasons"] and j["config"]["all_reduce"] == "torch.distributed"
    assert j["config"]["dist_backend"] == "gloo" and j["scaling"] == "weak" and np.isfinite(j["final_loss"])
    # without --allow-fallback: the same line, then a non-zero exit code on every rank
    procs, outs = run([])
    assert all(p.returncode == 3 for p in procs), [p.returncode for p in procs]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["fallback"] is True


@pytest.mark.gpu
def test_comm_init_is_bounded_when_a_rank_never_joins():
    """gmvae_comm_init (include/gmvae_hip.h): ncclCommInitRank blocks until every rank has joined -- the first real multi-GPU run
    must FAIL LOUDLY, not hang, if a peer died or the world sizes disagree.  A child process plays rank 0 of a 2-rank world whose
    rank 1 never arrives: the call comes back with GMVAE_E_TIMEOUT after GMVAE_COMM_INIT_TIMEOUT seconds and the child exits."""
    import subprocess
    import sys
    import time
    code = ("import ctypes as C, sys, torch\n"
            "torch.cuda.set_device(0)\n"
            "from gmvae_amd import _lib as L\n"
            "buf = C.create_string_buffer(128)\n"
            "assert L.lib.gmvae_comm_unique_id(L.rccl_path(), buf) == 0\n"
            "comm = C.c_void_p()\n"
            "rc = L.lib.gmvae_comm_init(L.rccl_path(), buf, 0, 2, C.byref(comm))\n"
            "print('rc', rc, flush=True)\n"
            "import os; os._exit(0 if rc == -7 else 1)\n")
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GMVAE_COMM_INIT_TIMEOUT="4", PYTHONPATH=ROOT)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "rc -7" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-600:])
    assert 3.0 < time.time() - t0 < 390                    # (a first `import torch` on a fresh box can take minutes)
