"""gmvae_posterior_y (include/gmvae_hip.h): the GMVAE's own posterior over its component y by importance sampling per
component -- l_bk = logsumexp_s log w'_bsk - ln n, r_b = softmax_k l_bk, and the row's bound, H(r), KL(q || r) and effective
sample size -- against the fp64 statement (tests/ymarg_ref.py) on its own Philox noise, against its own outputs recomputed in
fp64, against gmvae_iw_bound_enum_y's bound, against the y-summed-out importance-weighted objective (-L_b = bound_b -
KL(q_b || r_b)), at n = 1, K = 1, K = 80 and n = 5000, invariant under the chunk, the batch, the sharding and the engine's
objective, through predict_clusters and run_eval, and its error codes."""
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
SHAPES = {      # the shapes of tests/test_iw_enum.py, and one with more components than a wave has lanes
    "h24x2": O.Dims(D=100, L=5, K=7, hidden=(24, 24)),
    "defaults": O.Dims(D=784, L=64, K=10, hidden=(64,)),
    "k1": O.Dims(D=784, L=8, K=1, hidden=(64,)),
    "tanh": O.Dims(D=200, L=16, K=7, hidden=(64, 64), act="tanh"),
    "bias_vec": O.Dims(D=784, L=8, K=10, hidden=(64,), gen_bias_init=np.linspace(-2.0, 1.0, 784)),
    "h512": O.Dims(D=784, L=128, K=10, hidden=(512,)),
    "k80": O.Dims(D=100, L=8, K=80, hidden=(24,)),
}
FP64_SHAPES = ["h24x2", "defaults", "tanh", "bias_vec", "h512", "k80"]
ARGMAX_SHAPES = ["h24x2", "defaults", "tanh"]


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


def post(d, flat, x, n, chunk, row0=0, flags=0, seed=SEED, step=STEP):
    """One gmvae_posterior_y call: dict(log_joint [B, K], log_post [B, K], stats [B, 4], tail [8]) as numpy."""
    return hip_util.chunked_call("posterior_y", O.MODEL_GMVAE, d, flat, x, n, chunk, row0, flags, seed, step)


def enum_bound(d, flat, x, n, chunk, row0=0, seed=SEED, step=STEP):
    """gmvae_iw_bound_enum_y's bound_out [B] at the same dims."""
    return hip_util.chunked_call("iw_bound_enum_y", O.MODEL_GMVAE, d, flat, x, n, chunk, row0, seed=seed, step=step,
                                 omit=("mean_logw",))["bound"]


def forward(d, flat, x, S, flag, row0=0, seed=SEED, step=STEP):
    """gmvae_forward under an objective bit (GMVAE_OBJ_MARGINAL_Y at S = 1, GMVAE_OBJ_MARGINAL_Y_IW at any S) with in-kernel
    noise: (tail [8], rows [B S K, 4], logits [B, K]) as numpy."""
    return hip_util.forward_call(O.MODEL_GMVAE, d, flat, x, S, row0=row0, flags=flag, seed=seed, step=step, logits=True)


def log_softmax(v):
    v = np.asarray(v, np.float64)
    return v - lse(v, axis=1)[:, None]


def ess_of(lw):
    """(sum w)^2 / sum w^2 of w = exp(lw), over all of lw, in fp64."""
    lw = np.asarray(lw, np.float64).ravel()
    return float(np.exp(2.0 * lse(lw) - lse(2.0 * lw)))


_REF = {}


def fp64_log_w(name, d, flat, x, n, row0=0):
    """log w'_bsk [B, n, K] of the fp64 statement: per batch row b the n copies of x_b on oracle.noise(n K, ...,
    row_base=(row0 + b) n K), whose row s K + k is sample (s, k)."""
    key = (name, n, row0, x.shape[0], x.tobytes()[:64])
    if key not in _REF:
        p64 = O.unpack(O.MODEL_GMVAE, d, flat.astype(np.float64))
        out = []
        for b in range(x.shape[0]):
            eps = O.noise(n * d.K, d.L, d.K, (row0 + b) * n * d.K, SEED, STEP)[0]
            Cb, _ = YM.loss_and_grads(d, p64, np.repeat(x[b:b + 1], n, 0), eps)
            out.append(Cb["rows"][:, 3].reshape(n, d.K))
        _REF[key] = np.array(out)
    return _REF[key]


@pytest.mark.parametrize("name", FP64_SHAPES)
@pytest.mark.parametrize("n", [1, 37, 200])
def test_posterior_matches_the_fp64_statement(name, n):
    d, B = SHAPES[name], 8
    flat, x = _setup(d, B)
    lw = fp64_log_w(name, d, flat, x, n)                             # [B, n, K]
    ref_lj = lse(lw, axis=1) - np.log(n)                             # [B, K]
    ref_lp = log_softmax(ref_lj)
    ref_ess = np.array([ess_of(lw[b]) for b in range(B)])
    delta = 1e-4 * np.abs(lw).reshape(B, -1).max(1)                  # each log w' moves by at most delta: ESS by e^{+-4 delta}
    for chunk in (1, 5, n, n + 7):
        o = post(d, flat, x, n, chunk)
        lj, lp, ess = o["log_joint"].astype(np.float64), o["log_post"].astype(np.float64), o["stats"][:, 3].astype(np.float64)
        print(name, n, chunk, "log_joint rel", (np.abs(lj - ref_lj) / np.abs(ref_lj)).max(), "log_post abs",
              np.abs(lp - ref_lp).max(), "gate", (2e-4 * np.abs(ref_lj).max(1)).min(), "ess ratio", (ess / ref_ess).min(),
              (ess / ref_ess).max(), "ess", ess.min(), ess.max())
        assert np.all(np.abs(lj - ref_lj) <= 1e-4 * np.abs(ref_lj)), (chunk, lj, ref_lj)
        assert np.all(np.abs(lp - ref_lp) <= 2e-4 * np.abs(ref_lj).max(1, keepdims=True)), (chunk, lp, ref_lp)
        assert np.all(np.abs(np.log(ess / ref_ess)) <= 4 * delta), (chunk, ess, ref_ess)
        assert np.all(ess >= 1) and np.all(ess <= n * d.K)


def _check_self_consistent(o, logits, B, K):
    """The call's log_post, bound, entropy and KL recomputed in fp64 from its own fp32 log_joint and the forward's logits."""
    lj = o["log_joint"].astype(np.float64)
    bound = lse(lj, axis=1)
    lr = lj - bound[:, None]
    r = np.exp(lr)
    lnq = log_softmax(logits)
    q = np.exp(lnq)
    tol = dict(rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(o["log_post"], lr, **tol)
    np.testing.assert_allclose(o["stats"][:, 0], bound, **tol)
    np.testing.assert_allclose(o["stats"][:, 1], -(r * lr).sum(1), **tol)
    np.testing.assert_allclose(o["stats"][:, 2], (q * (lnq - lr)).sum(1), **tol)
    assert np.all(np.abs(np.exp(o["log_post"].astype(np.float64)).sum(1) - 1.0) <= 1e-6)
    s = o["stats"].astype(np.float64)
    sums = np.array([-s[:, 0].sum(), s[:, 1].sum(), s[:, 2].sum(), s[:, 3].sum()])
    t = o["tail"].astype(np.float64)
    assert np.all(np.abs(t[:4] - sums) <= 1e-5 * np.abs(sums)), (t, sums)
    assert t[4] == B and np.all(t[5:] == 0)


@pytest.mark.parametrize("name", ["h24x2", "defaults", "tanh", "k80"])
def test_outputs_are_consistent_with_each_other_and_with_the_enumerated_bound(name):
    d, B, n, row0 = SHAPES[name], 8, 37, 5
    flat, x = _setup(d, B, seed=1)
    _, _, logits = forward(d, flat, x, 1, _L().OBJ_MARGINAL_Y, row0=row0)     # the schedule the chunks run: the same logits
    for chunk in (1, 5, n):
        o = post(d, flat, x, n, chunk, row0=row0)
        _check_self_consistent(o, logits, B, d.K)
        eb = enum_bound(d, flat, x, n, chunk, row0=row0)                       # the same row bits, folded in another order
        np.testing.assert_allclose(o["stats"][:, 0], eb, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,n", [("h24x2", 6), ("defaults", 4), ("k80", 3)])
def test_bound_minus_kl_is_the_importance_weighted_objective_with_y_summed_out(name, n):
    """-L_b = bound_b - KL(q_b || r_b) for GMVAE_OBJ_MARGINAL_Y_IW's L_b at S = n on the same noise: sum_k q_k (ln q_k - l_k +
    bound) = KL, so bound - KL = sum_k q_k l_k - sum_k q_k ln q_k."""
    d, B, row0 = SHAPES[name], 8, 3
    flat, x = _setup(d, B, seed=2)
    ftail, rows, _ = forward(d, flat, x, n, _L().OBJ_MARGINAL_Y_IW, row0=row0)
    o = post(d, flat, x, n, n, row0=row0)
    s = o["stats"].astype(np.float64)
    want = -(s[:, 0] - s[:, 2]).sum()
    assert abs(ftail[0] - want) <= 1e-5 * abs(want), (ftail[0], want)
    lw = rows[:, 3].astype(np.float64).reshape(B, n * d.K)
    np.testing.assert_allclose(s[:, 3], [ess_of(r) for r in lw], rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", ["h24x2", "defaults", "tanh", "k80"])
def test_one_sample_is_the_marginal_forward(name):
    d, B, row0 = SHAPES[name], 6, 3
    flat, x = _setup(d, B, seed=1)
    _, rows, _ = forward(d, flat, x, 1, _L().OBJ_MARGINAL_Y, row0=row0)       # noise row (row0 + b) K + k: the same draws
    o = post(d, flat, x, 1, 1, row0=row0)
    np.testing.assert_allclose(o["log_joint"], rows[:, 3].reshape(B, d.K), rtol=1e-6, atol=0)


def test_k1_has_a_trivial_posterior_and_the_gumbel_bound():
    """K = 1: r = [1]; the same Philox rows ((row0 + b) n + s) and y = [1] as gmvae_iw_bound."""
    import torch
    d = SHAPES["k1"]
    B, n = 6, 37
    flat, x = _setup(d, B, seed=4)
    L = _L()
    o = post(d, flat, x, n, 5, row0=2)
    assert np.all(o["log_post"] == 0) and np.all(o["stats"][:, 1] == 0) and np.all(o["stats"][:, 2] == 0)
    cd = dims_of(dataclasses.replace(d, S=5), B)
    cd.row0 = 2
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, dtype=torch.float32, device="cuda")
    gb, gt = torch.zeros(B, device="cuda"), torch.zeros(L.TAIL, device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), O.MODEL_GMVAE, L.ptr(xd), L.ptr(params), n, L.ptr(gb), None, L.ptr(gt),
                                 L.ptr(ws), SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    np.testing.assert_allclose(o["log_joint"][:, 0], gb.cpu().numpy(), rtol=1e-5, atol=0)
    assert np.all(o["stats"][:, 3] >= 1) and np.all(o["stats"][:, 3] <= n)


def test_5000_samples_through_a_small_chunk():
    d = SHAPES["defaults"]
    B, n = 16, 5000
    flat, x = _setup(d, B, seed=3)
    o = post(d, flat, x, n, 7)
    assert all(np.all(np.isfinite(v)) for v in o.values())
    ess = o["stats"][:, 3]
    assert np.all(ess >= 1) and np.all(ess <= n * d.K)


@pytest.mark.parametrize("name", ["h24x2", "defaults"])
def test_posterior_is_invariant_under_chunk_batch_shards_and_flag(name):
    d = SHAPES[name]
    B, n = 8, 120
    flat, x = _setup(d, B, seed=2)
    L = _L()
    full, again = post(d, flat, x, n, 50), post(d, flat, x, n, 50)
    assert all(np.array_equal(full[k], again[k]) for k in full)
    flagged = post(d, flat, x, n, 50, flags=L.OBJ_MARGINAL_Y)          # the bit is ignored: the same bits
    assert all(np.array_equal(full[k], flagged[k]) for k in full)
    h = B // 2
    lo = post(d, flat, x[:h], n, 50, row0=0)["log_joint"]
    hi = post(d, flat, x[h:], n, 50, row0=h)["log_joint"]
    one = post(d, flat, x[h - 1:h + 1], n, 50, row0=h - 1)["log_joint"]
    # the general schedule's GEMM tilings (and so their fp32 summation order) follow the batch size
    np.testing.assert_allclose(np.concatenate([lo, hi]), full["log_joint"], rtol=1e-5, atol=0)
    np.testing.assert_allclose(one, full["log_joint"][h - 1:h + 1], rtol=1e-5, atol=0)
    for chunk in (1, 7, n):
        np.testing.assert_allclose(post(d, flat, x, n, chunk)["log_joint"], full["log_joint"], rtol=1e-5, atol=0)


def test_gumbel_and_marginal_engines_give_the_same_bits():
    import torch
    from gmvae_amd.engine import Engine
    eg = Engine("gmvae", 784, 64, 10, [64], random_seed=5)
    em = Engine("gmvae", 784, 64, 10, [64], random_seed=5, y_inference="marginal")
    ei = Engine("gmvae", 784, 64, 10, [64], random_seed=5, y_inference="marginal_iw", n_samples=3)
    with torch.no_grad():
        em.params.copy_(eg.params)
        ei.params.copy_(eg.params)
    x = torch.from_numpy((np.random.default_rng(9).random((24, 784)) < 0.87).astype(np.uint8)).cuda()
    a = eg.posterior_y(x, 30, chunk=7)
    assert set(a) == {"log_joint", "log_post", "bound", "entropy", "kl_q_post", "ess", "tail"}
    assert a["log_joint"].shape == (24, 10) and a["log_post"].shape == (24, 10) and a["tail"].shape == (8,)
    for e in (em, ei):
        b = e.posterior_y(x, 30, chunk=7)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.allclose(a["bound"], eg.iw_bound_enum_y(x, 30, chunk=7)["bound"], rtol=1e-6, atol=0)
    d = eg.posterior_y(x, 30)                                           # the default chunk
    assert torch.allclose(d["log_joint"], a["log_joint"], rtol=1e-5, atol=0)
    with pytest.raises(ValueError, match="VAE"):
        Engine("vae", 784, 8, 1, [64], random_seed=1).posterior_y(x, 4)
    with pytest.raises(ValueError, match="n_samples"):
        eg.posterior_y(x, 0)
    with pytest.raises(ValueError, match="chunk"):
        eg.posterior_y(x, 4, chunk=0)


@pytest.mark.parametrize("name", ARGMAX_SHAPES)
@pytest.mark.parametrize("n", [1, 37])
def test_predict_clusters_is_the_fp64_argmax(name, n):
    """On every row whose fp64 top-two gap in ln r exceeds log_post's tolerance (2e-4 max_k |l_bk|); at most 1/4 of the rows may
    lie inside it."""
    import torch
    from gmvae_amd.gmvae import create_gmvae
    d, B = SHAPES[name], 8
    flat, x = _setup(d, B)
    lw = fp64_log_w(name, d, flat, x, n)
    ref_lj = lse(lw, axis=1) - np.log(n)
    ref_lp = log_softmax(ref_lj)
    top = np.sort(ref_lp, axis=1)
    gap, tol = top[:, -1] - top[:, -2], 2e-4 * np.abs(ref_lj).max(1)
    clear = gap > tol
    print(name, n, "gap", gap, "tol", tol)
    assert (~clear).sum() <= B // 4
    model = create_gmvae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden),
                         hidden_activation_fn=getattr(torch, d.act), sigma_min=d.sigma_min, raw_sigma_bias=d.raw_sigma_bias,
                         gen_bias_init=d.gen_bias_init, temperature=d.temperature, random_seed=SEED)
    e = model._engine
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(flat[:e.P]))
    e.noise_seed, e.global_step = SEED, STEP
    pred = model.predict_clusters(torch.from_numpy(x).cuda(), n)
    assert pred.dtype == torch.int64 and pred.shape == (B,)
    lp = model.posterior_y(torch.from_numpy(x).cuda(), n)
    assert lp.shape == (B, d.K) and torch.equal(lp.argmax(dim=1), pred)
    assert np.array_equal(pred.cpu().numpy()[clear], ref_lp.argmax(1)[clear])


def _acc(logits, labels, K):
    """sum_k max_l hist[k, l] / N of the argmax clusters."""
    hist = np.zeros((K, 10), np.int64)
    np.add.at(hist, (np.asarray(logits).argmax(1), np.asarray(labels)), 1)
    return hist.max(1).sum() / len(labels)


@pytest.mark.parametrize("y_inference", ["gumbel", "marginal"])
def test_run_eval_reports_the_posterior_independent_of_batch_size(tmp_path, y_inference):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=gmvae", "--latent_size=64", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200", f"--y_inference={y_inference}"]
    run_gmvae.main(["--mode=train", "--batch_size=40"] + args)
    res = {bs: run_gmvae.main(["--mode=eval", f"--batch_size={bs}", "--posterior_samples=64"] + args) for bs in (16, 40)}
    cfg = run_gmvae.build_parser().parse_args(["--mode=eval", "--batch_size=200"] + args)
    model = runners.create_model(cfg, 784)
    model.load_state_dict(torch.load(runners._ckpt(cfg), map_location="cpu"))
    (images, labels), = list(runners.create_dataset(cfg, "train", shuffle=False, repeat=False))
    whole = model._engine.posterior_y(images, 64, row0=0)
    q_logits = model.encoder_y(images).distribution.logits.cpu().numpy()
    scale = whole["log_joint"].abs().max().item()
    for r in res.values():
        lp, st = r["log_posterior_y"], r["posterior_y_stats"].double()
        assert r["examples"] == 200 and lp.shape == (200, 10) and st.shape == (200, 4)
        assert torch.equal(r["labels"], labels)
        assert r["train/posterior_entropy_64_per_example"] == pytest.approx(st[:, 1].mean().item(), rel=1e-6)
        assert r["train/kl_q_posterior_64_per_example"] == pytest.approx(st[:, 2].mean().item(), rel=1e-6)
        assert r["train/ess_64_per_example"] == pytest.approx(st[:, 3].mean().item(), rel=1e-6)
        assert r["train/cluster_acc_posterior_64"] == pytest.approx(_acc(lp.cpu().numpy(), r["labels"].cpu().numpy(), 10), abs=1e-6)
        assert r["train/cluster_acc_q"] == pytest.approx(_acc(q_logits, r["labels"].cpu().numpy(), 10), abs=1e-6)
        assert (lp - whole["log_post"]).abs().max().item() <= 2e-5 * scale
    assert (res[16]["log_posterior_y"] - res[40]["log_posterior_y"]).abs().max().item() <= 2e-5 * scale
    plain = run_gmvae.main(["--mode=eval", "--batch_size=40"] + args)
    assert not [k for k in plain if "posterior" in k or "cluster_acc" in k or "/ess_" in k]


def test_error_codes_on_device_buffers():
    import torch
    L = _L()
    d = SHAPES["h24x2"]
    B = 4
    flat, x = _setup(d, B)
    cd = dims_of(dataclasses.replace(d, S=3), B)
    ws = torch.zeros(L.posterior_y_workspace_bytes(cd, O.MODEL_GMVAE) // 4 + 64, dtype=torch.float32, device="cuda")
    buf = torch.zeros(256, device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)

    def call(dims, model=O.MODEL_GMVAE, n=10, lj=None, w=None, tail=None):
        return L.lib.gmvae_posterior_y(C.byref(dims), model, L.ptr(xd), L.ptr(params), n,
                                       L.ptr(buf) if lj is None else lj, L.ptr(buf[64:]), L.ptr(buf[128:]),
                                       L.ptr(buf[192:]) if tail is None else tail, L.ptr(ws if w is None else w), SEED, STEP,
                                       L.current_stream())

    assert call(cd, n=0) == -2
    far = dims_of(dataclasses.replace(d, S=3), B)
    far.row0 = (1 << 38) // (1000 * d.K)
    assert call(far, n=1000) == -2
    big = dims_of(dataclasses.replace(d, S=1 << 8), 1 << 20)           # B S K = 7 * 2^28 > 2^30
    assert call(big) == -2
    for model in (O.MODEL_VAE, O.MODEL_VAE_GMP):
        assert call(cd, model=model) == -3
    assert call(cd, lj=C.c_void_p(buf.data_ptr() + 4)) == -4
    assert call(cd, tail=C.c_void_p(buf.data_ptr() + 4)) == -4
    assert call(cd, w=ws[1:]) == -4
    torch.cuda.synchronize()
    assert torch.all(buf == 0)                                          # nothing was launched
    assert call(cd) == 0                                                # ... and the same buffers pass
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:B * d.K]).all() and buf[192 + 4] == B
