"""gmvae_iw_bound_enum_y (include/gmvae_hip.h): the GMVAE's importance-weighted bound with y summed out exactly over its K
components, streamed in chunks -- against the fp64 statement (tests/ymarg_ref.py) on its own Philox noise, against the marginal
gmvae_forward at n = 1, invariant under the chunk, the batch, the sharding and the engine's objective, equal to gmvae_iw_bound
at K = 1, at n = 5000, through run_eval for a Gumbel- and a marginal-trained checkpoint, and its error codes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import oracle as O
import ymarg_ref as YM
import hip_util
from hip_util import dev, dims_of, lse

pytestmark = pytest.mark.gpu

SEED, STEP = 11, 3
SHAPES = {      # all on the general schedule (the enumerated bound has no one-launch form)
    "h24x2": O.Dims(D=100, L=5, K=7, hidden=(24, 24)),
    "defaults": O.Dims(D=784, L=64, K=10, hidden=(64,)),
    "k1": O.Dims(D=784, L=8, K=1, hidden=(64,)),
    "tanh": O.Dims(D=200, L=16, K=7, hidden=(64, 64), act="tanh"),
    "bias_vec": O.Dims(D=784, L=8, K=10, hidden=(64,), gen_bias_init=np.linspace(-2.0, 1.0, 784)),
    "h512": O.Dims(D=784, L=128, K=10, hidden=(512,)),
}


def _L():
    from gmvae_amd import _lib
    return _lib


def _setup(d, B, seed=0):
    p = O.init_params(O.MODEL_GMVAE, d, np.random.default_rng(seed))
    for k in p:                                   # non-zero biases: a q(y|x) away from uniform
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.3, p[k].shape)
    flat = O.pack(O.MODEL_GMVAE, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, O.MODEL_GMVAE, seed_x=100 + seed)
    return flat, x


def enum(d, flat, x, n, chunk, row0=0, flags=0, seed=SEED, step=STEP):
    """One gmvae_iw_bound_enum_y call: (bound [B], mean_logw [B], tail [8]) as numpy."""
    o = hip_util.chunked_call("iw_bound_enum_y", O.MODEL_GMVAE, d, flat, x, n, chunk, row0, flags, seed, step)
    return o["bound"], o["mean_logw"], o["tail"]


_REF = {}


def fp64_bound(name, d, flat, x, n, row0=0):
    """Per batch row b, the fp64 statement on the n copies of x_b with oracle.noise(n K, ..., row_base=(row0 + b) n K): its row
    s K + k is sample (s, k).  (bound = logsumexp rows[:, 3] - ln n, mean_logw = -loss) as arrays [B]."""
    key = (name, n, row0, x.shape[0])
    if key not in _REF:
        p64 = O.unpack(O.MODEL_GMVAE, d, flat.astype(np.float64))
        bs, ms = [], []
        for b in range(x.shape[0]):
            eps = O.noise(n * d.K, d.L, d.K, (row0 + b) * n * d.K, SEED, STEP)[0]
            Cb, _ = YM.loss_and_grads(d, p64, np.repeat(x[b:b + 1], n, 0), eps)
            bs.append(lse(Cb["rows"][:, 3]) - np.log(n))
            ms.append(-Cb["loss"])
        _REF[key] = (np.array(bs), np.array(ms))
    return _REF[key]


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("n", [1, 37, 200])
def test_enum_bound_matches_the_fp64_statement(name, n):
    d = SHAPES[name]
    flat, x = _setup(d, 5)
    ref, ref_mlw = fp64_bound(name, d, flat, x, n)
    assert np.all(ref_mlw <= ref)
    for chunk in (1, 5, n, n + 7):
        bound, mlw, tail = enum(d, flat, x, n, chunk)
        assert np.all(np.abs(bound - ref) <= 1e-4 * np.abs(ref)), (chunk, bound, ref)
        assert np.all(np.abs(mlw - ref_mlw) <= 1e-4 * np.abs(ref_mlw)), (chunk, mlw, ref_mlw)
        assert np.all(mlw <= bound)                                   # Gibbs per sample, then log-mean-exp >= mean
        assert tail[4] == 5 and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * abs(tail[0])
        assert np.all(tail[5:] == 0)


def _marginal_forward(d, flat, x, row0, seed=SEED, step=STEP):
    """gmvae_forward under GMVAE_OBJ_MARGINAL_Y with in-kernel noise: (tail [8], rows [B K, 4], logits [B, K])."""
    return hip_util.forward_call(O.MODEL_GMVAE, d, flat, x, 1, row0=row0, flags=_L().OBJ_MARGINAL_Y, seed=seed, step=step,
                                 logits=True)


@pytest.mark.parametrize("name", ["h24x2", "defaults", "tanh"])
def test_one_sample_is_the_marginal_forward(name):
    d, B, row0 = SHAPES[name], 6, 3
    flat, x = _setup(d, B, seed=1)
    ftail, rows, logits = _marginal_forward(d, flat, x, row0)        # noise row (row0 + b) K + k: the same draws
    lg = logits.astype(np.float64)
    lnq = lg - lg.max(1, keepdims=True)
    lnq -= np.log(np.exp(lnq).sum(1, keepdims=True))
    q = np.exp(lnq)
    lw = rows[:, 3].astype(np.float64).reshape(B, d.K)
    neg_L = (q * lw).sum(1) - (q * lnq).sum(1)                          # -L_b of the marginal objective
    # chunk 1: the marginal forward itself; chunk 4: the same rows inside a 4-sample pass (other GEMM tilings)
    for chunk, tol in ((1, 1e-6), (4, 1e-5)):
        bound, mlw, tail = enum(d, flat, x, 1, chunk, row0=row0)
        assert np.allclose(mlw, neg_L, rtol=tol, atol=0), (chunk, mlw, neg_L)
        assert np.allclose(bound, [lse(r) for r in lw], rtol=tol, atol=0)
        assert np.allclose(tail[1:5], ftail[1:5], rtol=tol, atol=tol * np.abs(ftail[1:5]).max()), (chunk, tail, ftail)


@pytest.mark.parametrize("name", ["h24x2", "defaults"])
def test_enum_bound_is_invariant_under_chunk_batch_shards_and_flag(name):
    d = SHAPES[name]
    B, n = 8, 120
    flat, x = _setup(d, B, seed=2)
    L = _L()
    full, mfull, tfull = enum(d, flat, x, n, 50)
    again, magain, tagain = enum(d, flat, x, n, 50)
    assert np.array_equal(full, again) and np.array_equal(mfull, magain) and np.array_equal(tfull, tagain)
    flagged = enum(d, flat, x, n, 50, flags=L.OBJ_MARGINAL_Y)          # the bit is ignored: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(flagged, (full, mfull, tfull)))
    h = B // 2
    lo, _, _ = enum(d, flat, x[:h], n, 50, row0=0)
    hi, _, _ = enum(d, flat, x[h:], n, 50, row0=h)
    one, _, _ = enum(d, flat, x[h - 1:h + 1], n, 50, row0=h - 1)
    # the general schedule's GEMM tilings (and so their fp32 summation order) follow the batch size
    assert np.allclose(np.concatenate([lo, hi]), full, rtol=1e-5, atol=0)
    assert np.allclose(one, full[h - 1:h + 1], rtol=1e-5, atol=0)
    for chunk in (1, 7, n):
        got, mgot, _ = enum(d, flat, x, n, chunk)
        assert np.allclose(got, full, rtol=1e-5, atol=0) and np.allclose(mgot, mfull, rtol=1e-5, atol=0)


def test_gumbel_and_marginal_engines_give_the_same_bits():
    import torch
    from gmvae_amd.engine import Engine
    eg = Engine("gmvae", 784, 64, 10, [64], random_seed=5)
    em = Engine("gmvae", 784, 64, 10, [64], random_seed=5, y_inference="marginal")
    with torch.no_grad():
        em.params.copy_(eg.params)
    assert (eg.noise_seed, eg.global_step) == (em.noise_seed, em.global_step)
    x = torch.from_numpy((np.random.default_rng(9).random((24, 784)) < 0.87).astype(np.uint8)).cuda()
    a, b = eg.iw_bound_enum_y(x, 30, chunk=7), em.iw_bound_enum_y(x, 30, chunk=7)
    for k in ("bound", "mean_logw", "tail"):
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="marginal"):                   # unchanged: the Gumbel bound refuses a marginal engine
        em.iw_bound(x, 30)
    with pytest.raises(ValueError, match="VAE"):
        Engine("vae", 784, 8, 1, [64], random_seed=1).iw_bound_enum_y(x, 4)


@pytest.mark.parametrize("name", ["k1"])
def test_k1_is_the_gumbel_bound(name):
    """K = 1: the same Philox rows ((row0 + b) n + s), y = [1] in both, nent = 0."""
    import torch
    d = SHAPES[name]
    B, n = 6, 37
    flat, x = _setup(d, B, seed=4)
    L = _L()
    bound, mlw, tail = enum(d, flat, x, n, 5, row0=2)
    cd = dims_of(dataclasses.replace(d, S=5), B)
    cd.row0 = 2
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, dtype=torch.float32, device="cuda")
    gb, gm, gt = (torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(L.TAIL, device="cuda"))
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), L.ptr(params), n, L.ptr(gb), L.ptr(gm), L.ptr(gt),
                                 L.ptr(ws), SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    assert np.allclose(bound, gb.cpu().numpy(), rtol=1e-5, atol=0)
    assert np.allclose(mlw, gm.cpu().numpy(), rtol=1e-5, atol=0)
    assert tail[3] == 0 and np.allclose(tail[:5], gt.cpu().numpy()[:5], rtol=1e-5, atol=1e-5)


def test_5000_samples_through_a_small_chunk():
    d = SHAPES["defaults"]
    B, n = 16, 5000
    flat, x = _setup(d, B, seed=3)
    bound, mlw, tail = enum(d, flat, x, n, 7)
    assert np.all(np.isfinite(bound)) and np.all(np.isfinite(mlw)) and np.all(np.isfinite(tail))
    assert np.all(mlw <= bound)


def test_error_codes_on_device_buffers():
    import torch
    L = _L()
    d = SHAPES["h24x2"]
    B = 4
    flat, x = _setup(d, B)
    cd = dims_of(dataclasses.replace(d, S=3), B)
    ws = torch.zeros(L.iw_bound_enum_y_workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, dtype=torch.float32, device="cuda")
    buf = torch.zeros(64, device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)

    def call(dims, model=O.MODEL_GMVAE, n=10, bound=None, w=None):
        return L.lib.gmvae_iw_bound_enum_y(C.byref(dims), model, L.ptr(xd), L.ptr(params), n,
                                           L.ptr(buf) if bound is None else bound, None, L.ptr(buf[16:]),
                                           L.ptr(ws if w is None else w), SEED, STEP, L.current_stream())

    assert call(cd, n=0) == -2
    far = dims_of(dataclasses.replace(d, S=3), B)
    far.row0 = (1 << 38) // (1000 * d.K)
    assert call(far, n=1000) == -2
    big = dims_of(dataclasses.replace(d, S=1 << 8), 1 << 20)           # B S K = 7 * 2^28 > 2^30
    assert call(big) == -2
    for model in (O.MODEL_VAE, O.MODEL_VAE_GMP):
        assert call(cd, model=model) == -3
    assert call(cd, bound=C.c_void_p(buf.data_ptr() + 4)) == -4
    assert call(cd, w=ws[1:]) == -4
    torch.cuda.synchronize()
    mcd = dims_of(dataclasses.replace(d, S=1), B)
    mcd.sched_flags = L.OBJ_MARGINAL_Y
    assert L.lib.gmvae_iw_bound(C.byref(mcd), O.MODEL_GMVAE, L.ptr(xd), L.ptr(params), 10, None, None, L.ptr(buf[16:]),
                                L.ptr(ws), SEED, STEP, L.current_stream()) == -2


@pytest.mark.parametrize("y_inference", ["gumbel", "marginal"])
def test_run_eval_reports_the_enum_bound_independent_of_batch_size(tmp_path, y_inference):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", "--latent_size=64", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200", f"--y_inference={y_inference}"]
    run_gmvae.main(["--mode=train", "--batch_size=40"] + args)
    res = {bs: run_gmvae.main(["--mode=eval", f"--batch_size={bs}", "--iw_enum_samples=64"] + args) for bs in (16, 40)}
    key = "train/iw_bound_enum_y_64_per_example"
    for r in res.values():
        assert r["examples"] == 200 and r["iw_bounds_enum_y"].shape == (200,)
        assert r[key] == pytest.approx(r["iw_bounds_enum_y"].double().mean().item(), rel=1e-6)
    assert torch.allclose(res[16]["iw_bounds_enum_y"], res[40]["iw_bounds_enum_y"], rtol=1e-5, atol=0)
    # the mean of model.iw_bound_enum_y over the split as ONE batch (row0 = 0: example i's draws start at Philox row i n K)
    cfg = run_gmvae.build_parser().parse_args(["--mode=eval", "--batch_size=200"] + args)
    model = runners.create_model(cfg, 784)
    model.load_state_dict(torch.load(runners._ckpt(cfg), map_location="cpu"))
    (images, _), = list(runners.create_dataset(cfg, "train", shuffle=False, repeat=False))
    whole = model.iw_bound_enum_y(images, 64)
    assert torch.allclose(whole, res[16]["iw_bounds_enum_y"], rtol=1e-5, atol=0)
    assert res[16][key] == pytest.approx(whole.double().mean().item(), rel=1e-6)
