"""gmvae_posterior_component (include/gmvae_hip.h): the VAE_GMP's own posterior over the component k of its learned mixture prior
by importance sampling -- l_bk = logsumexp_s log w_bsk - ln n, r_b = softmax_k l_bk, and the row's bound, H(r), KL(r || pi) and
effective sample size -- against the fp64 statement (tests/post_comp_ref.py) on its own Philox noise, against its own outputs
recomputed in fp64, against gmvae_iw_bound's bound on both schedules, against the one-sample forward, with the mixture pulled far
apart, at K = 1, K = 80 and n = 5000, invariant under the chunk, the batch and the sharding, through predict_clusters and
run_eval, and its error codes.

Invariance (test_posterior_is_invariant_...): at the reference's default sizes (csrc/evalf.hpp: a sample row's chain never mixes
with other rows, and the fold is fp64 from the first exp on) log_joint is asserted BIT-EQUAL under the chunk, the batch split,
the shards and a second call.  On the general schedule two calls are bit-equal too, but the forward's GEMM tilings -- and so the
fp32 summation order of every log w -- follow the number of rows B S of the pass, exactly as for gmvae_iw_bound
(tests/test_iw_bound.py), so there the chunk and the batch split are held to that test's rtol 1e-5."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import oracle as O
import post_comp_ref as R
import hip_util
from hip_util import dev, dims_of

pytestmark = pytest.mark.gpu

M = O.MODEL_VAE_GMP
SEED, STEP = 11, 3
SHAPES = {
    "defaults": O.Dims(D=784, L=64, K=10, hidden=(64,)),              # csrc/evalf.hpp: one launch per chunk
    "h24x2": O.Dims(D=100, L=5, K=7, hidden=(24, 24)),
    "tanh": O.Dims(D=200, L=16, K=7, hidden=(64, 64), act="tanh"),
    "bias_vec": O.Dims(D=784, L=8, K=10, hidden=(64,), gen_bias_init=np.linspace(-2.0, 1.0, 784)),
    "h512": O.Dims(D=784, L=128, K=10, hidden=(512,)),
    "k80": O.Dims(D=100, L=8, K=80, hidden=(24,)),
    "k1": O.Dims(D=784, L=8, K=1, hidden=(64,)),
}
FP64_SHAPES = ["defaults", "h24x2", "tanh", "bias_vec", "h512", "k80", "k1"]
ARGMAX_SHAPES = ["defaults", "h24x2", "tanh"]


def _L():
    from gmvae_amd import _lib
    return _lib


def _setup(d, B, seed=0):
    p = O.init_params(M, d, np.random.default_rng(seed))
    for k in p:                                   # non-zero biases
        if k.endswith("/b"):
            p[k] = np.random.default_rng(seed + 7).normal(0, 0.3, p[k].shape)
    p["mixture_logits"] = np.random.default_rng(seed + 9).normal(0, 1.0, p["mixture_logits"].shape)      # a non-uniform pi
    flat = O.pack(M, d, p, np.float32)
    x, _, _ = O.make_inputs(d, B, M, seed_x=100 + seed)
    return flat, x


def post(d, flat, x, n, chunk, row0=0, seed=SEED, step=STEP):
    """One gmvae_posterior_component call: dict(log_joint [B, K], log_post [B, K], stats [B, 4], tail [8]) as numpy."""
    return hip_util.chunked_call("posterior_component", M, d, flat, x, n, chunk, row0, seed=seed, step=step)


def iw_bound(d, flat, x, n, chunk, row0=0, seed=SEED, step=STEP):
    """gmvae_iw_bound's bound_out [B] at the same dims."""
    return hip_util.chunked_call("iw_bound", M, d, flat, x, n, chunk, row0, seed=seed, step=step, omit=("mean_logw",))["bound"]


def forward_rows(d, flat, x, row0=0, seed=SEED, step=STEP):
    """gmvae_forward at S = 1 with in-kernel noise (Philox row row0 + b): rows [B, 4] as numpy."""
    return hip_util.forward_call(M, d, flat, x, 1, row0=row0, seed=seed, step=step)[1]


_REF = {}


def fp64_log_w(name, flat, x, n, row0=0):
    key = (name, n, row0, x.shape[0], flat.tobytes()[:256], x.tobytes()[:64])
    if key not in _REF:
        _REF[key] = R.log_w(SHAPES[name], flat, x, n, row0, SEED, STEP)
    return _REF[key]


def _check_fp64(name, o, lw, n, what):
    """Gate 1 of the statement: |l - ref| <= 1e-4 |ref|; |ln r - ref| <= 2e-4 max_k |ref l|; |ln(ESS / ref)| <= 4e-4 max |log w|;
    1 <= ESS <= n."""
    B = lw.shape[0]
    ref = R.statement(lw)
    delta = 1e-4 * np.abs(lw).reshape(B, -1).max(1)                  # each log w moves by at most delta: ESS by e^{+-4 delta}
    lj, lp, ess = o["log_joint"].astype(np.float64), o["log_post"].astype(np.float64), o["stats"][:, 3].astype(np.float64)
    print(name, n, what, "log_joint rel", (np.abs(lj - ref["log_joint"]) / np.abs(ref["log_joint"])).max(), "log_post abs",
          np.abs(lp - ref["log_post"]).max(), "gate", (2e-4 * np.abs(ref["log_joint"]).max(1)).min(), "ess ratio",
          (ess / ref["ess"]).min(), (ess / ref["ess"]).max(), "ess", ess.min(), ess.max())
    assert all(np.all(np.isfinite(v)) for v in o.values())
    assert np.all(np.abs(lj - ref["log_joint"]) <= 1e-4 * np.abs(ref["log_joint"])), (what, lj, ref["log_joint"])
    assert np.all(np.abs(lp - ref["log_post"]) <= 2e-4 * np.abs(ref["log_joint"]).max(1, keepdims=True)), (what, lp, ref["log_post"])
    assert np.all(np.abs(np.log(ess / ref["ess"])) <= 4 * delta), (what, ess, ref["ess"])
    assert np.all(ess >= 1) and np.all(ess <= n)


@pytest.mark.parametrize("name", FP64_SHAPES)
@pytest.mark.parametrize("n", [1, 37, 200])
def test_posterior_matches_the_fp64_statement(name, n):
    d, B = SHAPES[name], 8
    flat, x = _setup(d, B)
    lw = fp64_log_w(name, flat, x, n)                                # [B, n, K]
    for chunk in (1, 5, n, n + 7):
        _check_fp64(name, post(d, flat, x, n, chunk), lw, n, chunk)


def _check_self_consistent(o, mixlog, B, K):
    """The call's log_post, bound, entropy and KL recomputed in fp64 from its own fp32 log_joint and the parameters'
    mixture_logits."""
    lj = o["log_joint"].astype(np.float64)
    bound = R.lse(lj, axis=1)
    lr = lj - bound[:, None]
    r = np.exp(lr)
    lnpi = R.log_softmax(np.asarray(mixlog, np.float64).reshape(1, K))
    tol = dict(rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(o["log_post"], lr, **tol)
    np.testing.assert_allclose(o["stats"][:, 0], bound, **tol)
    np.testing.assert_allclose(o["stats"][:, 1], -(r * lr).sum(1), **tol)
    np.testing.assert_allclose(o["stats"][:, 2], (r * (lr - lnpi)).sum(1), **tol)
    assert np.all(np.abs(np.exp(o["log_post"].astype(np.float64)).sum(1) - 1.0) <= 1e-6)
    s = o["stats"].astype(np.float64)
    sums = np.array([-s[:, 0].sum(), s[:, 1].sum(), s[:, 2].sum(), s[:, 3].sum()])
    t = o["tail"].astype(np.float64)
    assert np.all(np.abs(t[:4] - sums) <= 1e-5 * np.abs(sums)), (t, sums)
    assert t[4] == B and np.all(t[5:] == 0)


@pytest.mark.parametrize("no_evalf", [False, True])
@pytest.mark.parametrize("name", ["defaults", "h24x2", "tanh", "k80"])
def test_outputs_are_consistent_with_each_other_and_with_the_streamed_bound(name, no_evalf, monkeypatch):
    """... and bound_b IS gmvae_iw_bound's on the same dims, n, row0, seed and step (rtol 1e-5: the logsumexp over k is taken in
    another place), on the one-launch schedule and with GMVAE_NO_EVALF=1."""
    if no_evalf:
        monkeypatch.setenv("GMVAE_NO_EVALF", "1")
    d, B, n, row0 = SHAPES[name], 8, 37, 5
    flat, x = _setup(d, B, seed=1)
    mixlog = O.unpack(M, d, flat.astype(np.float64))["mixture_logits"]
    for chunk in (1, 5, n):
        o = post(d, flat, x, n, chunk, row0=row0)
        _check_self_consistent(o, mixlog, B, d.K)
        np.testing.assert_allclose(o["stats"][:, 0], iw_bound(d, flat, x, n, chunk, row0=row0), rtol=1e-5, atol=0)


def test_the_default_sizes_take_the_one_launch_schedule(monkeypatch):
    """A/B on GMVAE_NO_EVALF: the general schedule multiplies in another arithmetic (fp32 GEMM tiles against evalf.hpp's bf16
    piece products), so the two agree to rounding and not in their bits -- the default call is not the general loop."""
    d, B, n = SHAPES["defaults"], 8, 37
    flat, x = _setup(d, B, seed=1)
    a = post(d, flat, x, n, 5)
    monkeypatch.setenv("GMVAE_NO_EVALF", "1")
    b = post(d, flat, x, n, 5)
    np.testing.assert_allclose(a["log_joint"], b["log_joint"], rtol=1e-5, atol=0)
    assert not np.array_equal(a["log_joint"], b["log_joint"])


@pytest.mark.parametrize("name", ["defaults", "h24x2", "tanh", "k80"])
def test_one_sample_is_the_forward(name):
    """n = 1: logsumexp_k log_joint is gmvae_forward's log w at S = 1 on the same Philox row."""
    d, B, row0 = SHAPES[name], 6, 3
    flat, x = _setup(d, B, seed=1)
    rows = forward_rows(d, flat, x, row0=row0)
    o = post(d, flat, x, 1, 1, row0=row0)
    np.testing.assert_allclose(R.lse(o["log_joint"], axis=1), rows[:, 3], rtol=1e-5, atol=0)
    assert np.all(o["stats"][:, 3] == 1)


def test_k1_has_a_trivial_posterior():
    d, B, n = SHAPES["k1"], 6, 37
    flat, x = _setup(d, B, seed=4)
    o = post(d, flat, x, n, 5, row0=2)
    assert np.all(o["log_post"] == 0) and np.all(o["stats"][:, 1] == 0) and np.all(o["stats"][:, 2] == 0)
    np.testing.assert_allclose(o["log_joint"][:, 0], iw_bound(d, flat, x, n, 5, row0=2), rtol=1e-5, atol=0)
    assert np.all(o["stats"][:, 3] >= 1) and np.all(o["stats"][:, 3] <= n)


@pytest.mark.parametrize("no_evalf", [False, True])
@pytest.mark.parametrize("name", ["defaults", "h24x2", "k80"])
def test_separated_mixture_stays_in_the_log_domain(name, no_evalf, monkeypatch):
    """loc spread over +-8 at s ~ 0.05: comp_k - logsumexp is below -1000 for most k (where a responsibility is 0 even in fp64).
    Every output is finite and l_bk holds gate 1 for the far components too."""
    if no_evalf:
        monkeypatch.setenv("GMVAE_NO_EVALF", "1")
    d, B, n = SHAPES[name], 8, 37
    flat, x = _setup(d, B, seed=5)
    flat = R.separate(d, flat)
    lw = fp64_log_w(name, flat, x, n)
    assert np.all(np.isfinite(lw)) and ((lw - R.lse(lw, axis=2)[:, :, None]) < -1000).mean() > 0.5
    for chunk in (5, n):
        _check_fp64(name, post(d, flat, x, n, chunk), lw, n, chunk)


def test_5000_samples_through_a_small_chunk():
    d = SHAPES["defaults"]
    B, n = 16, 5000
    flat, x = _setup(d, B, seed=3)
    o = post(d, flat, x, n, 7)
    assert all(np.all(np.isfinite(v)) for v in o.values())
    ess = o["stats"][:, 3]
    assert np.all(ess >= 1) and np.all(ess <= n)


@pytest.mark.parametrize("name", ["defaults", "h24x2"])
def test_posterior_is_invariant_under_chunk_batch_and_shards(name):
    d = SHAPES[name]
    B, n = 8, 120
    flat, x = _setup(d, B, seed=2)
    full, again = post(d, flat, x, n, 50), post(d, flat, x, n, 50)
    assert all(np.array_equal(full[k], again[k]) for k in full)       # fixed-order folds, one owner per (b, k): the same bits
    h = B // 2
    lo = post(d, flat, x[:h], n, 50, row0=0)["log_joint"]             # two virtual shards with their row offsets
    hi = post(d, flat, x[h:], n, 50, row0=h)["log_joint"]
    one = post(d, flat, x[h - 1:h + 1], n, 50, row0=h - 1)["log_joint"]      # a batch of two rows from the middle
    chunks = [post(d, flat, x, n, chunk)["log_joint"] for chunk in (1, 5, n)]
    if name == "defaults":                                            # (the module docstring: why bit-equal here, rtol below)
        assert np.array_equal(np.concatenate([lo, hi]), full["log_joint"])
        assert np.array_equal(one, full["log_joint"][h - 1:h + 1])
        for c in chunks:
            assert np.array_equal(c, full["log_joint"])
    else:
        np.testing.assert_allclose(np.concatenate([lo, hi]), full["log_joint"], rtol=1e-5, atol=0)
        np.testing.assert_allclose(one, full["log_joint"][h - 1:h + 1], rtol=1e-5, atol=0)
        for c in chunks:
            np.testing.assert_allclose(c, full["log_joint"], rtol=1e-5, atol=0)


def test_engine_posterior_component():
    import torch
    from gmvae_amd.engine import Engine
    e = Engine("vae_gmp", 784, 64, 10, [64], random_seed=5)
    x = torch.from_numpy((np.random.default_rng(9).random((24, 784)) < 0.87).astype(np.uint8)).cuda()
    a = e.posterior_component(x, 30, chunk=7)
    assert set(a) == {"log_joint", "log_post", "bound", "entropy", "kl_post_prior", "ess", "tail"}
    assert a["log_joint"].shape == (24, 10) and a["log_post"].shape == (24, 10) and a["tail"].shape == (8,)
    assert torch.allclose(a["bound"], e.iw_bound(x, 30, chunk=7)["bound"], rtol=1e-5, atol=0)
    assert torch.equal(e.posterior_component(x, 30)["log_joint"], a["log_joint"])       # the default chunk
    for other in (Engine("vae", 784, 8, 1, [64], random_seed=1), Engine("gmvae", 784, 8, 10, [64], random_seed=1)):
        with pytest.raises(ValueError, match="vae_gmp"):
            other.posterior_component(x, 4)
    with pytest.raises(ValueError, match="VAE"):                       # posterior_y stays the GMVAE's
        e.posterior_y(x, 4)
    with pytest.raises(ValueError, match="n_samples"):
        e.posterior_component(x, 0)
    with pytest.raises(ValueError, match="chunk"):
        e.posterior_component(x, 4, chunk=0)


ARGMAX_SEED = {"defaults": 0, "h24x2": 0, "tanh": 0}


@pytest.mark.parametrize("name", ARGMAX_SHAPES)
@pytest.mark.parametrize("n", [1, 37])
def test_predict_clusters_is_the_fp64_argmax(name, n):
    """On every row whose fp64 top-two gap in ln r exceeds log_post's tolerance (2e-4 max_k |l_bk|).  At most 1 row in 8 may lie
    inside it; at these seeds the fp64 reference leaves out no row at all (gap and tolerance are printed; checked on the CPU)."""
    import torch
    from gmvae_amd.vae import create_vae
    d, B = SHAPES[name], 8
    flat, x = _setup(d, B, seed=ARGMAX_SEED[name])
    ref = R.statement(fp64_log_w(name, flat, x, n))
    top = np.sort(ref["log_post"], axis=1)
    gap, tol = top[:, -1] - top[:, -2], 2e-4 * np.abs(ref["log_joint"]).max(1)
    clear = gap > tol
    print(name, n, "gap", gap, "tol", tol, "rows left out", int((~clear).sum()))
    assert (~clear).sum() <= B // 8
    model = create_vae(d.D, d.L, mixture_components=d.K, fcnet_hidden_sizes=list(d.hidden),
                       hidden_activation_fn=getattr(torch, d.act), sigma_min=d.sigma_min, raw_sigma_bias=d.raw_sigma_bias,
                       gen_bias_init=d.gen_bias_init, random_seed=SEED)
    e = model._engine
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(flat[:e.P]))
    e.noise_seed, e.global_step = SEED, STEP
    pred = model.predict_clusters(torch.from_numpy(x).cuda(), n)
    assert pred.dtype == torch.int64 and pred.shape == (B,)
    lp = model.posterior_component(torch.from_numpy(x).cuda(), n)
    assert lp.shape == (B, d.K) and torch.equal(lp.argmax(dim=1), pred)
    assert np.array_equal(pred.cpu().numpy()[clear], ref["log_post"].argmax(1)[clear])
    with pytest.raises(ValueError, match="vae_gmp"):                   # the plain VAE has no components
        create_vae(d.D, d.L, fcnet_hidden_sizes=list(d.hidden)).predict_clusters(torch.from_numpy(x).cuda(), n)


def _acc(logits, labels, K):
    """sum_k max_l hist[k, l] / N of the argmax clusters."""
    hist = np.zeros((K, 10), np.int64)
    np.add.at(hist, (np.asarray(logits).argmax(1), np.asarray(labels)), 1)
    return hist.max(1).sum() / len(labels)


def test_run_eval_reports_the_posterior_independent_of_batch_size(tmp_path):
    import torch
    from gmvae_amd import run_gmvae, runners
    args = ["--model=vae_gmp", "--latent_size=64", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200"]
    run_gmvae.main(["--mode=train", "--batch_size=40"] + args)
    res = {bs: run_gmvae.main(["--mode=eval", f"--batch_size={bs}", "--component_posterior_samples=64"] + args) for bs in (16, 40)}
    cfg = run_gmvae.build_parser().parse_args(["--mode=eval", "--batch_size=200"] + args)
    model = runners.create_model(cfg, 784)
    model.load_state_dict(torch.load(runners._ckpt(cfg), map_location="cpu"))
    (images, labels), = list(runners.create_dataset(cfg, "train", shuffle=False, repeat=False))
    whole = model._engine.posterior_component(images, 64, row0=0)
    for r in res.values():
        lp, st = r["log_posterior_component"], r["posterior_component_stats"].double()
        assert r["examples"] == 200 and lp.shape == (200, 10) and st.shape == (200, 4)
        assert torch.equal(r["labels"], labels)
        assert r["train/posterior_entropy_64_per_example"] == pytest.approx(st[:, 1].mean().item(), rel=1e-6)
        assert r["train/kl_posterior_prior_64_per_example"] == pytest.approx(st[:, 2].mean().item(), rel=1e-6)
        assert r["train/ess_64_per_example"] == pytest.approx(st[:, 3].mean().item(), rel=1e-6)
        assert r["train/cluster_acc_posterior_64"] == pytest.approx(_acc(lp.cpu().numpy(), r["labels"].cpu().numpy(), 10), abs=1e-6)
        assert torch.equal(lp, whole["log_post"])                       # per example, whatever the batch: the same bits
    assert torch.equal(res[16]["log_posterior_component"], res[40]["log_posterior_component"])
    for k in ("train/cluster_acc_posterior_64", "train/posterior_entropy_64_per_example", "train/kl_posterior_prior_64_per_example",
              "train/ess_64_per_example"):
        assert res[16][k] == pytest.approx(res[40][k], rel=1e-6)
    plain = run_gmvae.main(["--mode=eval", "--batch_size=40"] + args)
    assert set(plain) == set(res[40]) - {k for k in res[40] if "posterior" in k or "cluster_acc" in k or "/ess_" in k}
    assert not [k for k in plain if "posterior" in k or "cluster_acc" in k or "/ess_" in k]


def test_error_codes_on_device_buffers():
    import torch
    L = _L()
    d = SHAPES["h24x2"]
    B = 4
    flat, x = _setup(d, B)
    cd = dims_of(dataclasses.replace(d, S=3), B)
    ws = torch.zeros(L.posterior_component_workspace_bytes(cd, M) // 4 + 64, dtype=torch.float32, device="cuda")
    buf = torch.zeros(256, device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)

    def call(dims, model=M, n=10, lj=None, w=None, tail=None):
        return L.lib.gmvae_posterior_component(C.byref(dims), model, L.ptr(xd), L.ptr(params), n,
                                               L.ptr(buf) if lj is None else lj, L.ptr(buf[64:]), L.ptr(buf[128:]),
                                               L.ptr(buf[192:]) if tail is None else tail, L.ptr(ws if w is None else w), SEED,
                                               STEP, L.current_stream())

    assert call(cd, n=0) == -2
    far = dims_of(dataclasses.replace(d, S=3), B)
    far.row0 = (1 << 38) // 1000
    assert call(far, n=1000) == -2
    big = dims_of(dataclasses.replace(d, S=1 << 11), 1 << 20)          # B S = 2^31 > 2^30
    assert call(big) == -2
    for model in (O.MODEL_VAE, O.MODEL_GMVAE):
        assert call(cd, model=model) == -3
    assert call(cd, lj=C.c_void_p(buf.data_ptr() + 4)) == -4
    assert call(cd, tail=C.c_void_p(buf.data_ptr() + 4)) == -4
    assert call(cd, w=ws[1:]) == -4
    torch.cuda.synchronize()
    assert torch.all(buf == 0)                                          # nothing was launched
    assert call(cd) == 0                                                # ... and the same buffers pass
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:B * d.K]).all() and buf[192 + 4] == B
