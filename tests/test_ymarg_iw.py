"""The importance-weighted objective with y summed out (include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y_IW, csrc/ymarg.hpp
ymarg_iw_rows) on the device: the step against the fp64 statement (tests/ymarg_iw_ref.py) at the gates of
hip_util.compare_step, S = 1 against the marginal step bit for bit, K = 1 against the Gumbel IWAE step, the in-kernel noise
against gmvae_noise_fill, row shards, the forward outputs, the bound sandwich against gmvae_iw_bound_enum_y on the same noise,
train graphs (eager vs captured, pipeline, data parallel with a one-rank communicator), an 8-step trajectory, the error codes
and the runner end to end."""
import ctypes as C
import dataclasses
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import ymarg_iw_ref as YI
from hip_util import _L, check_grads, dev, dims_of, drop_comm, hip_step, tail_gates

pytestmark = pytest.mark.gpu

LR = 1e-3
SIZES = {       # name: (Dims, B, S)
    "run_gmvae_defaults_s2": (O.Dims(D=784, L=8, K=10, hidden=(64,)), 16, 2),
    "run_gmvae_defaults_s5": (O.Dims(D=784, L=8, K=10, hidden=(64,)), 16, 5),
    "configs2_s2": (O.Dims(D=784, L=64, K=10, hidden=(64,)), 1024, 2),
    "k64": (O.Dims(D=784, L=32, K=64, hidden=(64,)), 64, 2),
    "k80": (O.Dims(D=200, L=8, K=80, hidden=(64,)), 16, 2),
    "s100_k3": (O.Dims(D=100, L=5, K=3, hidden=(24,)), 8, 100),
    "h64x64_tanh": (O.Dims(D=200, L=16, K=7, hidden=(64, 64), act="tanh"), 24, 3),
    "bias_vec": (O.Dims(D=784, L=8, K=10, hidden=(64,), gen_bias_init=np.linspace(-2.0, 1.0, 784)), 16, 2),
}
DEF = O.Dims(D=784, L=8, K=10, hidden=(64,))


def _idims(d, B, S, row0=0, flags=None):
    cd = dims_of(dataclasses.replace(d, S=S), B)
    cd.sched_flags = _L().OBJ_MARGINAL_Y_IW if flags is None else flags
    cd.row0 = row0
    return cd


def _setup(d, B, S, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.05, p[k].shape)
    flat = O.pack(O.MODEL_GMVAE, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    eps = np.random.default_rng(seed + 1).standard_normal((B * S * d.K, d.L)).astype(np.float32)
    return flat, x, eps


def istep(d, S, flat, x, eps, row0=0, seed=5, step=3, flags=None):
    """One gmvae_step with the objective bit: (grad sums [P] float64, tail [8], the step's ReLU masks)."""
    return hip_step(O.MODEL_GMVAE, dataclasses.replace(d, S=S), flat, x, eps, None, seed, step, want_masks=True,
                    flags=_L().OBJ_MARGINAL_Y_IW if flags is None else flags, row0=row0, mask_rows=S * d.K)


def compare_step(d, S, flat, x, eps, what, row0=0, grad_rtol=1e-4):
    B = x.shape[0]
    p32 = O.unpack(O.MODEL_GMVAE, d, flat.astype(np.float64))
    gs, tail, masks = istep(d, S, flat, x, eps, row0=row0)
    Cc, g = YI.loss_and_grads(d, p32, x, eps, S)
    tail_gates(what, tail, B, Cc)
    check_grads(what, O.MODEL_GMVAE, d, gs, g, B, masks, Cc["pre"], lambda m: YI.loss_and_grads(d, p32, x, eps, S, relu_masks=m)[1],
                grad_rtol)
    return gs, tail, Cc


@pytest.mark.parametrize("name", list(SIZES))
def test_step_matches_fp64_statement(name):
    d, B, S = SIZES[name]
    flat, x, eps = _setup(d, B, S, seed=len(name))
    compare_step(d, S, flat, x, eps, name)


def test_one_sample_is_the_marginal_step_bit_for_bit():
    import torch
    L = _L()
    d, B = DEF, 16
    flat, x, eps = _setup(d, B, 1, seed=2)
    for e in (eps, None):
        g8, t8, _ = istep(d, 1, flat, x, e)
        g4, t4, _ = istep(d, 1, flat, x, e, flags=L.OBJ_MARGINAL_Y)
        assert np.array_equal(g8, g4) and np.array_equal(t8, t4)
    a = _engine(d, 21, n_samples=1)
    b = _engine(d, 21, y_inference="marginal")
    xs = torch.from_numpy((np.random.default_rng(3).random((3, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    for t in range(3):
        a.train_step(xs[t], lr=LR)
        b.train_step(xs[t], lr=LR)
    torch.cuda.synchronize()
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v), (a.grads, b.grads)):
        assert torch.equal(u.detach(), v.detach())


@pytest.mark.parametrize("S", [2, 7])
def test_k1_is_the_gumbel_iwae_step(S):
    """K = 1: y = [1] in both objectives, q = 1, nent = 0; row (b S + s) K + k = b S + s draws the same eps."""
    d = O.Dims(D=784, L=8, K=1, hidden=(64,))
    B = 32
    flat, x, eps = _setup(d, B, S, seed=4)
    gi, ti, _ = istep(d, S, flat, x, eps)
    u = np.full((B * S, 1), 0.5, np.float32)
    gg, tg = hip_step(O.MODEL_GMVAE, dataclasses.replace(d, S=S), flat, x, eps, u)
    np.testing.assert_allclose(ti[:5], tg[:5], rtol=2e-5, atol=1e-4)
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        n = int(np.prod(shape))
        ref = gg[off:off + n]
        assert np.abs(gi[off:off + n] - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-6), name


def test_in_kernel_noise_is_noise_fill_and_shards_add_up():
    """eps = NULL draws gmvae_noise_fill's rows at row_base = row0 * S * K; two row shards add up to the whole batch."""
    import torch
    L = _L()
    d, S = DEF, 3
    B = 16
    flat, x, _ = _setup(d, B, S, seed=3)
    row0, seed, step = 48, 5, 3
    g0, t0, _ = istep(d, S, flat, x, None, row0=row0, seed=seed, step=step)
    R = B * S * d.K
    eps = torch.zeros(R, d.L, dtype=torch.float32, device="cuda")
    L.check(L.lib.gmvae_noise_fill(L.ptr(eps), None, R, d.L, d.K, row0 * S * d.K, seed, step, None, L.current_stream()),
            "gmvae_noise_fill")
    torch.cuda.synchronize()
    e = eps.cpu().numpy()
    g1, t1, _ = istep(d, S, flat, x, e, row0=row0, seed=seed, step=step)
    assert np.array_equal(g0, g1) and np.array_equal(t0, t1)
    compare_step(d, S, flat, x, e, "row0", row0=row0)
    B = 64
    flat, x, _ = _setup(d, B, S, seed=4)
    gf, tf, _ = istep(d, S, flat, x, None)
    ga, ta, _ = istep(d, S, flat, x[:B // 2], None, row0=0)
    gb, tb, _ = istep(d, S, flat, x[B // 2:], None, row0=B // 2)
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
    d, B, S = DEF, 16, 3
    flat, x, eps = _setup(d, B, S, seed=6)
    R = B * S * d.K
    cd = _idims(d, B, S)
    params, xd, ed = dev(flat, torch.float32), dev(x, torch.uint8), dev(eps, torch.float32)
    f32 = dict(dtype=torch.float32, device="cuda")
    tail, rows, z = torch.zeros(L.TAIL, **f32), torch.zeros(R, 4, **f32), torch.zeros(R, d.L, **f32)
    y, lg = torch.zeros(R, d.K, **f32), torch.zeros(B, d.K, **f32)
    ws = torch.zeros(L.workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, **f32)
    L.check(L.lib.gmvae_forward(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), L.ptr(ed), None, L.ptr(params), L.ptr(tail), L.ptr(rows),
                                L.ptr(z), L.ptr(y), L.ptr(lg), L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    tail, rows, z, y, lg = (t.cpu().numpy().astype(np.float64) for t in (tail, rows, z, y, lg))
    _, ts, Cc = compare_step(d, S, flat, x, eps, "forward")
    np.testing.assert_allclose(tail[:5], ts[:5], rtol=1e-6)
    tail_gates("forward", tail, B, Cc)
    np.testing.assert_allclose(rows, Cc["rows"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(z, Cc["z"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(lg, Cc["logits"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(y, np.tile(np.eye(d.K), (B * S, 1)))


def _engine(d, seed, y_inference="marginal_iw", **kw):
    from gmvae_amd.engine import Engine
    return Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=seed, y_inference=y_inference, **kw)


def _neg_L(o, B, S, K):
    """-L_b from a forward's rows and logits (fp64 on the host)."""
    lw = o["rows"][:, 3].double().cpu().view(B, S, K)
    lnq = o["logits"].double().cpu().log_softmax(dim=1)
    q = lnq.exp()
    import torch
    ell = -(torch.logsumexp(lw, dim=1) - np.log(S))
    return (-((q * ell).sum(1) + (q * lnq).sum(1))).numpy()


@pytest.mark.parametrize("S", [1, 4])
def test_bound_sandwich_on_the_same_noise(S):
    import torch
    d, B = DEF, 64
    e = _engine(d, 31, n_samples=S)
    e.global_step = 7
    x = torch.from_numpy(_setup(d, B, S, seed=8)[1]).cuda()
    o = e.forward(x)
    b = e.iw_bound_enum_y(x, S, chunk=S)
    torch.cuda.synchronize()
    neg = _neg_L(o, B, S, d.K)
    np.testing.assert_allclose(neg.sum(), -o["tail"][0].item(), rtol=1e-5)
    bound, mlw = b["bound"].double().cpu().numpy(), b["mean_logw"].double().cpu().numpy()
    slack = 1e-5 * np.abs(neg) + 1e-3
    assert (mlw <= neg + slack).all() and (neg <= bound + slack).all()
    if S == 1:
        np.testing.assert_allclose(mlw, neg, rtol=1e-5, atol=1e-3)
    else:
        assert (neg - mlw).mean() > 1e-3
    # the bound does not depend on the engine's objective: a Gumbel engine with the same parameters and noise keys
    g = _engine(d, 31, y_inference="gumbel")
    g.global_step = 7
    bg = g.iw_bound_enum_y(x, S, chunk=S)
    for k in ("bound", "mean_logw", "tail"):
        assert torch.equal(b[k], bg[k]), k


def test_engine_api():
    import torch
    from gmvae_amd import gmvae
    d, B, S = DEF, 16, 3
    e = _engine(d, 1, n_samples=S)
    assert e.rows_per_x == S * d.K
    x = torch.from_numpy(_setup(d, B, S)[1]).cuda()
    o = e.forward(x)
    R = B * S * d.K
    assert o["rows"].shape == (R, 4) and o["z"].shape == (R, d.L) and o["y"].shape == (R, d.K)
    assert o["logits"].shape == (B, d.K)
    o2 = e.forward(x, n_samples=2)
    assert o2["rows"].shape == (B * 2 * d.K, 4)
    with pytest.raises(ValueError):
        e.step(x, u=torch.rand(B * S, d.K))
    with pytest.raises(ValueError):
        e.step(x, eps=torch.zeros(B * d.K, d.L))              # eps has B*S*K rows
    with pytest.raises(ValueError, match="marginal_iw"):
        e.iw_bound(x, 10)
    assert e.iw_bound_enum_y(x, 6)["bound"].shape == (B,)
    loss = e.loss(x, torch.zeros(R, d.L))
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(e.params.grad).all()
    # checkpoints load across all three modes
    m = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=2,
                           n_samples=S, y_inference="marginal_iw")
    for kw in (dict(), dict(y_inference="marginal")):
        g = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=3, **kw)
        g.load_state_dict(m.state_dict())
        assert torch.equal(g.params, m.params)
        m2 = gmvae.create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden), random_seed=4,
                                n_samples=2, y_inference="marginal_iw")
        m2.load_state_dict(g.state_dict())
        assert torch.equal(g.params, m2.params)


def test_error_codes():
    import torch
    L = _L()
    d, B, S = DEF, 16, 2
    flat, x, _ = _setup(d, B, S)
    xd, params = dev(x, torch.uint8), dev(flat, torch.float32)
    grads = torch.zeros(flat.size + L.TAIL, device="cuda")
    ws = torch.zeros(1 << 22, device="cuda")
    for model in (O.MODEL_VAE, O.MODEL_VAE_GMP):
        assert L.lib.gmvae_step(C.byref(_idims(d, B, S)), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws),
                                0, 0, None, L.current_stream()) == -3
    cd = _idims(d, B, 1, flags=L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW)
    assert L.lib.gmvae_step(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
                            L.current_stream()) == -2
    tail = torch.zeros(L.TAIL, device="cuda")
    assert L.lib.gmvae_iw_bound(C.byref(_idims(d, B, S)), O.MODEL_GMVAE, L.ptr(xd), L.ptr(params), 10, None, None, L.ptr(tail),
                                L.ptr(ws), 0, 0, L.current_stream()) == -2
    assert L.step_schedule(_idims(d, B, S), O.MODEL_GMVAE) == "general+marginal_iw"


def test_train_graph_is_eager_steps_bit_for_bit():
    import torch
    d, B = DEF, 16
    xs = torch.from_numpy((np.random.default_rng(8).random((4, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(d, 11, n_samples=3), _engine(d, 11, n_samples=3)
    for t in range(4):
        a.train_step(xs[t], lr=LR)
    sx, replay = b.capture_train_step(B, lr=LR, n_steps=4)
    sx.copy_(xs)
    replay()
    torch.cuda.synchronize()
    assert a.global_step == b.global_step == 4
    for u, v in ((a.params, b.params), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(u.detach(), v.detach())
    assert torch.equal(replay.tail_log[3], a.grads[a.P:])


def test_pipeline_graph_is_binarise_then_step():
    import torch
    from gmvae_amd.data import DeviceDataset, binarize
    from gmvae_amd.engine import Engine
    d, B = DEF, 16
    n = 3
    pix = np.random.default_rng(9).integers(0, 256, (300, d.D), dtype=np.uint8)
    a, b = _engine(d, 12, n_samples=2), _engine(d, 12, n_samples=2)
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
    d, B = DEF, 16
    xs = torch.from_numpy((np.random.default_rng(10).random((2, B, d.D)) < 0.87).astype(np.uint8)).cuda()
    a, b = _engine(d, 13, n_samples=2), _engine(d, 13, n_samples=2)
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
    """8 eager train steps on injected noise against 8 fp64 statement steps + oracle.adam_tf_step (fp64), as
    tests/test_ymarg.py does for the single-sample objective."""
    import torch
    d, B, S = O.Dims(D=100, L=5, K=7, hidden=(24, 24)), 8, 3
    n = 8
    e = _engine(d, 14, n_samples=S)
    flat0 = e.params.detach().cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(15)
    xs = (rng.random((n, B, d.D)) < 0.87).astype(np.uint8)
    epss = rng.standard_normal((n, B * S * d.K, d.L)).astype(np.float32)
    ref = flat0.copy()
    m, v = np.zeros_like(ref), np.zeros_like(ref)
    for t in range(n):
        pre = e.params.detach().cpu().numpy().astype(np.float64)
        tail = e.train_step(torch.from_numpy(xs[t]).cuda(), eps=torch.from_numpy(epss[t]).cuda(), lr=LR).cpu().numpy()
        Cd, _ = YI.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, pre), xs[t], epss[t], S)
        tail_gates(f"step {t}", tail.astype(np.float64), B, Cd)
        _, g = YI.loss_and_grads(d, O.unpack(O.MODEL_GMVAE, d, ref), xs[t], epss[t], S)
        ref, m, v = O.adam_tf_step(ref, m, v, O.pack(O.MODEL_GMVAE, d, g, np.float64), t + 1, lr=LR, dtype=np.float64)
    fin = e.params.detach().cpu().numpy().astype(np.float64)
    lay, _, _ = O.param_layout(O.MODEL_GMVAE, d)
    for name, shape, off in lay:
        k = int(np.prod(shape))
        dd, dr = fin[off:off + k] - flat0[off:off + k], ref[off:off + k] - flat0[off:off + k]
        assert np.linalg.norm(dd - dr) <= 0.02 * max(np.linalg.norm(dr), 1e-12), name


def test_runner_trains_and_evaluates(tmp_path):
    logdir = str(tmp_path / "run")
    common = [sys.executable, "-m", "gmvae_amd.run_gmvae", f"--logdir={logdir}", "--y_inference=marginal_iw", "--n_samples=3",
              "--random_seed=3", "--synthetic_size=2048", "--batch_size=64"]
    r = subprocess.run(common + ["--mode=train", "--max_steps=300", "--summarise_every=50"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    import glob
    import os
    import re
    assert glob.glob(os.path.join(logdir, "*")), "no checkpoint written"
    losses = [float(v) for v in re.findall(r"loss[^0-9\-]*(-?[0-9.]+(?:e[-+]?\d+)?)", r.stdout + r.stderr)]
    assert len(losses) >= 2 and all(np.isfinite(losses)) and losses[-1] < losses[0], (r.stdout[-2000:], r.stderr[-2000:])
    r = subprocess.run(common + ["--mode=eval", "--checkpoint_max_wait=5", "--iw_enum_samples=20"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for key in ("loss_per_example", "nll", "kl_div_z", "nent", "iw_bound_enum_y_20_per_example"):
        assert re.search(rf"train/{key}: (-?[0-9.]+)", r.stdout), (key, r.stdout[-2000:])
    neg_loss = -float(re.search(r"train/loss_per_example: (-?[0-9.e+\-]+)", r.stdout).group(1))
    bound = float(re.search(r"train/iw_bound_enum_y_20_per_example: (-?[0-9.e+\-]+)", r.stdout).group(1))
    assert np.isfinite(bound) and np.isfinite(neg_loss)
