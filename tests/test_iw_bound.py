"""gmvae_iw_bound (include/gmvae_hip.h): the importance-weighted bound at any number of samples, streamed in chunks -- against the
fp64 oracle on its own Philox noise, against the one-shot gmvae_forward, and invariant under the chunk, the batch and the sharding,
on both schedules (evalf.hpp's one launch per chunk at the reference's default sizes; noise fill + forward + iw_merge elsewhere)."""
import dataclasses

import numpy as np
import pytest

import oracle as O
import hip_util
from hip_util import dims_of

pytestmark = pytest.mark.gpu

SEED, STEP = 11, 3
SHAPES = {      # (model, dims): small shapes on the general schedule, the reference's default sizes on evalf.hpp
    "gmvae_small": (O.MODEL_GMVAE, O.Dims(D=100, L=5, K=7, hidden=(24, 24))),
    "vae_small": (O.MODEL_VAE, O.Dims(D=97, L=4, K=1, hidden=(16,))),
    "vae_gmp_small": (O.MODEL_VAE_GMP, O.Dims(D=60, L=3, K=4, hidden=(16,))),
    "gmvae_evalf": (O.MODEL_GMVAE, O.Dims(D=784, L=64, K=10, hidden=(64,))),
    "vae_evalf": (O.MODEL_VAE, O.Dims(D=784, L=2, K=1, hidden=(64,))),
    "vae_gmp_evalf": (O.MODEL_VAE_GMP, O.Dims(D=784, L=64, K=10, hidden=(64,))),
}


def _L():
    from gmvae_amd import _lib
    return _lib


def _setup(name, B, seed=0):
    model, d = SHAPES[name]
    p = O.init_params(model, d, np.random.default_rng(seed))
    flat = O.pack(model, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, model, seed_x=100 + seed)
    return model, d, flat, x


def iw(model, d, flat, x, n, chunk, row0=0, seed=SEED, step=STEP):
    """One gmvae_iw_bound call: (bound [B], mean_logw [B], tail [8]) as numpy."""
    o = hip_util.chunked_call("iw_bound", model, d, flat, x, n, chunk, row0, seed=seed, step=step)
    return o["bound"], o["mean_logw"], o["tail"]


def forward(model, d, flat, x, S, eps=None, u=None, row0=0, seed=SEED, step=STEP):
    """gmvae_forward at S samples (in-kernel noise when eps is None): (tail [8], rows [B S, 4])."""
    return hip_util.forward_call(model, d, flat, x, S, eps, u, row0, seed=seed, step=step)[:2]


def lse(lw):
    return hip_util.lse(lw, axis=-1) - np.log(np.shape(lw)[-1])


_REF = {}


def oracle_bound(name, model, d, flat, x, n, row0=0):
    """fp64 oracle per batch row b on oracle.noise(n, ..., row_base=(row0 + b) n): logsumexp_s log w - log n."""
    key = (name, n, row0, x.shape[0])
    if key not in _REF:
        p32 = O.unpack(model, d, flat.astype(np.float64))
        out = []
        for b in range(x.shape[0]):
            eps, u = O.noise(n, d.L, d.K, (row0 + b) * n, SEED, STEP)
            Cb = O.forward(model, dataclasses.replace(d, S=n), p32, x[b:b + 1], eps, u if model == O.MODEL_GMVAE else None)
            out.append(Cb["bound"][0])
        _REF[key] = np.array(out)
    return _REF[key]


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("n", [1, 37, 200])
def test_iw_bound_matches_the_oracle(name, n):
    model, d, flat, x = _setup(name, 5)
    ref = oracle_bound(name, model, d, flat, x, n)
    for chunk in (1, 5, n, n + 7):
        bound, mlw, tail = iw(model, d, flat, x, n, chunk)
        assert np.all(np.abs(bound - ref) <= 1e-4 * np.abs(ref)), (chunk, bound, ref)
        assert np.all(mlw <= bound + 1e-4 * np.abs(bound))            # Jensen: mean log w <= log mean w
        assert tail[4] == 5 and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * abs(tail[0])


@pytest.mark.parametrize("name", ["gmvae_small", "vae_gmp_small", "gmvae_evalf", "vae_evalf", "vae_gmp_evalf"])
def test_iw_bound_at_chunk_n_is_the_one_shot_forward(name):
    n, B = 40, 6
    model, d, flat, x = _setup(name, B, seed=1)
    bound, mlw, tail = iw(model, d, flat, x, n, n, row0=3)
    ftail, rows = forward(model, d, flat, x, n, row0=3)               # keying row0*S + b*S + s: the same draws
    lw = rows[:, 3].reshape(B, n)
    assert np.allclose(bound, lse(lw), rtol=1e-6, atol=0)
    assert np.allclose(mlw, lw.astype(np.float64).mean(axis=1), rtol=1e-6, atol=0)
    assert np.allclose(tail[:5], ftail[:5], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("no_evalf", [False, True])
@pytest.mark.parametrize("name", ["gmvae_evalf", "vae_gmp_evalf", "gmvae_small"])
def test_iw_bound_is_invariant_under_chunk_batch_and_shards(name, no_evalf, monkeypatch):
    if no_evalf:
        monkeypatch.setenv("GMVAE_NO_EVALF", "1")
    B, n = 8, 120
    model, d, flat, x = _setup(name, B, seed=2)
    full, mfull, tfull = iw(model, d, flat, x, n, 50)
    again, _, tagain = iw(model, d, flat, x, n, 50)
    assert np.array_equal(full, again) and np.array_equal(tfull, tagain)          # fixed-order merge: the same bits
    h = B // 2
    lo, _, _ = iw(model, d, flat, x[:h], n, 50, row0=0)
    hi, _, _ = iw(model, d, flat, x[h:], n, 50, row0=h)
    shards = np.concatenate([lo, hi])
    one, _, _ = iw(model, d, flat, x[h - 1:h + 1], n, 50, row0=h - 1)             # a batch of two rows from the middle
    if name.endswith("evalf") and not no_evalf:
        # evalf_rows: a sample row's chain never mixes with other rows, and a batch row's chunk is folded by one wave in a fixed
        # order: the row's bits do not depend on which rows share its launch
        assert np.array_equal(shards, full) and np.array_equal(one, full[h - 1:h + 1])
    else:
        # the general schedule's GEMM tilings (and so their fp32 summation order) follow the batch size
        assert np.allclose(shards, full, rtol=1e-5, atol=0) and np.allclose(one, full[h - 1:h + 1], rtol=1e-5, atol=0)
    for chunk in (7, 64, n):
        # not bit-identical across chunk sizes: within a chunk the sums are fp32 (evalf) and fold into fp64 chunk by chunk
        got, mgot, _ = iw(model, d, flat, x, n, chunk)
        assert np.allclose(got, full, rtol=1e-5, atol=0) and np.allclose(mgot, mfull, rtol=1e-5, atol=0)


def test_iw_bound_at_5000_samples_through_a_3200_row_workspace():
    name, B, n, chunk = "gmvae_evalf", 64, 5000, 50
    model, d, flat, x = _setup(name, B, seed=3)
    L = _L()
    cd = dims_of(dataclasses.replace(d, S=chunk), B)
    assert L.iw_bound_workspace_bytes(cd, model) < L.workspace_bytes(dims_of(dataclasses.replace(d, S=250), B), model)
    bound, _, _ = iw(model, d, flat, x, n, chunk)
    noise = [O.noise(n, d.L, d.K, b * n, SEED, STEP) for b in range(B)]
    lw = np.zeros((B, n))
    for k in range(20):                                   # twenty 250-sample one-shot forwards on the same strided draws
        sl = slice(250 * k, 250 * (k + 1))
        eps = np.concatenate([e[sl] for e, _ in noise])
        u = np.concatenate([u_[sl] for _, u_ in noise])
        _, rows = forward(model, d, flat, x, 250, eps, u)
        lw[:, sl] = rows[:, 3].reshape(B, 250)
    ref = lse(lw)
    assert np.all(np.abs(bound - ref) <= 1e-4 * np.abs(ref)), np.abs(bound - ref).max()


def test_run_eval_reports_the_iw_bound_independent_of_batch_size(tmp_path):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", "--latent_size=64", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200"]
    run_gmvae.main(["--mode=train", "--batch_size=40"] + args)
    res = {bs: run_gmvae.main(["--mode=eval", f"--batch_size={bs}", "--iw_samples=64"] + args) for bs in (16, 40)}
    key = "train/iw_bound_64_per_example"
    for r in res.values():
        assert r["examples"] == 200 and r["iw_bounds"].shape == (200,)
        assert r[key] == pytest.approx(r["iw_bounds"].double().mean().item(), rel=1e-6)
        assert r[key] >= -r["train/loss_per_example"] - 1e-3 * abs(r[key])          # more samples: a tighter bound (up to noise)
    assert torch.allclose(res[16]["iw_bounds"], res[40]["iw_bounds"], rtol=1e-5, atol=0)
    # the mean of model.iw_bound over the split, as ONE batch (row0 = 0: example i draws Philox rows i n .. i n + n - 1)
    cfg = run_gmvae.build_parser().parse_args(["--mode=eval", "--batch_size=200"] + args)
    model = runners.create_model(cfg, 784)
    model.load_state_dict(torch.load(runners._ckpt(cfg), map_location="cpu"))
    (images, _), = list(runners.create_dataset(cfg, "train", shuffle=False, repeat=False))
    whole = model.iw_bound(images, 64)
    assert torch.allclose(whole, res[16]["iw_bounds"], rtol=1e-5, atol=0)
    assert res[16][key] == pytest.approx(whole.double().mean().item(), rel=1e-6)
