"""gmvae_ais (include/gmvae_hip.h; csrc/ais.hpp) on the device against the fp64 statement (tests/ais_ref.py): parity of the accept
sequence, log w and z_T on the device's own noise over the three models, both bases, the activations, ragged sizes and the size
gates' corners; bit-equalities (in-kernel Philox against supplied noise, the batch split, the launch split, two calls); the T = 1
identities against Engine.forward and Engine.iw_bound; quadrature on a two-dimensional latent; stats and tail.

Parity holds the DECIDED chains of the statement (ais_ref.ais: every accept test, ReLU pre-activation and component pick clear of
its edge by the margins given there) to the accept sequence exactly and to 1e-4 max(1, |.|) in log w and z_T -- the project's ELBO
gate --, and a case may leave at most 10 % of its chains undecided.  The shares of the seeds below are in profiles/ais_notes.md."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ais_ref as R
import oracle as O
from hip_util import dev, dims_of

pytestmark = pytest.mark.gpu

MODELS = {"vae": O.MODEL_VAE, "vae_gmp": O.MODEL_VAE_GMP, "gmvae": O.MODEL_GMVAE}
TOL = 1e-4


def _L():
    from gmvae_amd import _lib
    return _lib


def make(model, d, B, seed, scale=2.0):
    """Xavier weights times `scale`, small random biases, x ~ Bernoulli(1/2): (params fp32-exact, flat, x)."""
    rng = np.random.default_rng(seed)
    p = {k: scale * v for k, v in O.init_params(model, d, rng).items()}
    for k in p:
        if k.endswith("/b"):
            p[k] = 0.1 * rng.standard_normal(p[k].shape)
    flat = O.pack(model, d, p)
    p = {k: v.astype(np.float64) for k, v in O.unpack(model, d, flat).items()}
    x = (rng.random((B, d.D)) < 0.5).astype(np.uint8)
    return p, flat, x


def device_noise(T, n, Lz, row_base, seed, step):
    """The draws gmvae_ais makes itself, as arrays: eps [T + 1, n, L], u [T + 1, n] (gmvae_noise_fill at step (T + 1) + t)."""
    L = _L()
    es, us = [], []
    for t in range(T + 1):
        e = torch.empty(n, Lz, dtype=torch.float32, device="cuda")
        u = torch.empty(n, 1, dtype=torch.float32, device="cuda")
        L.check(L.lib.gmvae_noise_fill(L.ptr(e), L.ptr(u), n, Lz, 1, row_base, seed, step * (T + 1) + t, None, L.current_stream()),
                "gmvae_noise_fill")
        es.append(e)
        us.append(u.reshape(n))
    return torch.stack(es).contiguous(), torch.stack(us).contiguous()


def device_ais(model, d, flat, x, betas, C_, n_leap, step0, base=None, eps=None, u=None, row0=0, seed=7, step=3, up=1.02,
               down=0.96):
    """One gmvae_ais call on fresh buffers: dict of numpy outputs and the accept records [B C] (uint64)."""
    L = _L()
    B = x.shape[0]
    cd = dims_of(d, B)
    cd.row0 = row0
    n, T = B * C_, len(betas) - 1
    base_K = 0 if base is None else base[0].shape[1]
    bd = None
    if base is not None:
        bd = dev(np.concatenate([np.asarray(a, np.float32).reshape(B, -1) for a in base], axis=1))
    nbytes = L.ais_workspace_bytes(cd, model, base_K, C_)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")      # (needs no initialisation)
    f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(logw=torch.empty(B, C_, **f32), bound=torch.empty(B, **f32), stats=torch.empty(B, 4, **f32),
             z=torch.empty(n, d.L, **f32), tail=torch.empty(L.TAIL, **f32))
    keep = (dev(flat), dev(x), dev(np.asarray(betas, np.float32)))
    rc = L.lib.gmvae_ais(C.byref(cd), model, L.ptr(keep[1]), L.ptr(keep[0]), L.ptr(bd), base_K, L.ptr(keep[2]), T, C_, n_leap,
                         step0, up, down, L.ptr(eps), L.ptr(u), L.ptr(o["logw"]), L.ptr(o["bound"]), L.ptr(o["stats"]),
                         L.ptr(o["z"]), L.ptr(o["tail"]), L.ptr(ws), seed, step, L.current_stream())
    L.check(rc, "gmvae_ais")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["bits"] = ws[:2 * n].cpu().numpy().view(np.uint64)
    return out


def accept_matrix(bits, T):
    return ((bits[None, :] >> np.arange(T, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)


# ----------------------------------------------------------------------------------------------------------------- 1. parity
# (model, init, act, D, L, K, hidden, B, C, T, n_leapfrog)
SMALL = dict(T=8, leap=3)
CASES = [
    ("gmvae", "prior", "relu", 24, 3, 4, (16,), 4, 16),
    ("gmvae", "encoder", "tanh", 23, 5, 3, (12, 20), 3, 5),
    ("gmvae", "encoder", "relu", 23, 3, 4, (), 3, 5),
    ("gmvae", "prior", "tanh", 24, 5, 4, (), 4, 16),
    ("gmvae", "prior", "relu", 23, 3, 5, (12, 20), 3, 5),
    ("vae", "prior", "relu", 23, 5, 1, (12, 20), 4, 16),
    ("vae", "encoder", "tanh", 24, 3, 1, (16,), 3, 5),
    ("vae", "encoder", "relu", 24, 5, 1, (), 4, 16),
    ("vae_gmp", "prior", "tanh", 23, 3, 4, (16,), 3, 5),
    ("vae_gmp", "encoder", "relu", 24, 5, 3, (12, 20), 4, 16),
    ("vae_gmp", "prior", "relu", 24, 3, 4, (), 3, 5),
    ("gmvae", "encoder", "elu", 23, 5, 3, (16,), 3, 5),
    ("vae_gmp", "prior", "sigmoid", 24, 3, 4, (12, 20), 3, 5),
    # every size gate's last admitted corner at once (and the largest LDS layout): 3 x 512, L = 128, K = base_K = 64
    ("gmvae", "encoder", "tanh", 23, 128, 64, (512, 512, 512), 2, 3, 2, 2),
    # bin/run_train.sh's sizes, D off a multiple of 4
    ("vae_gmp", "prior", "relu", 787, 128, 10, (512,), 1, 5, 2, 2),
    # the reference's defaults
    ("gmvae", "prior", "relu", 784, 64, 10, (64,), 2, 16, 2, 2),
    ("gmvae", "encoder", "relu", 784, 64, 10, (64,), 2, 16, 2, 2),
    # the gates' lower corners: one pixel; one pixel, one latent dimension, one component, one hidden unit
    ("vae", "prior", "tanh", 1, 3, 1, (16,), 3, 5),
    ("vae_gmp", "encoder", "tanh", 1, 1, 1, (1,), 3, 5),
]
cid = lambda c: "-".join(str(v).replace(" ", "") for v in c)


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_parity_against_the_statement(case):
    name, init, act, D, Lz, K, hidden, B, C_ = case[:9]
    T, leap = case[9:] if len(case) > 9 else (SMALL["T"], SMALL["leap"])
    model = MODELS[name]
    d = O.Dims(D=D, L=Lz, K=K, hidden=hidden, act=act, gen_bias_init=np.linspace(-0.5, 0.5, D).astype(np.float32) if D == 23 else 0.1)
    p, flat, x = make(model, d, B, 1000 + CASES.index(case))
    betas = R.schedule("sigmoid", T).astype(np.float32)
    base = None
    if init == "encoder":
        base = tuple(a.astype(np.float32) for a in R.encoder_table(model, d, p, x))
    eps, u = device_noise(T, B * C_, Lz, 0, 7, 3)
    got = device_ais(model, d, flat, x, betas, C_, leap, 0.5, base, eps, u)
    ref = R.ais(model, d, p, x, betas.astype(np.float64), C_, leap, 0.5, eps.cpu().numpy(), u.cpu().numpy(), init, base=base)
    dec = ref["decided"]
    acc = accept_matrix(got["bits"], T)
    rate = ref["accepts"].mean()
    print(f"{cid(case)}: undecided {int((~dec).sum())} of {dec.size}, accept rate {rate:.2f}, "
          f"max |dlogw| {np.abs(got['logw'].reshape(-1) - ref['logw'].reshape(-1))[dec].max(initial=0):.2e}")
    assert (~dec).mean() <= 0.10
    assert np.array_equal(acc[:, dec], ref["accepts"][:, dec])
    lw_g, lw_r = got["logw"].reshape(-1)[dec], ref["logw"].reshape(-1)[dec]
    assert np.all(np.abs(lw_g - lw_r) <= TOL * np.maximum(1.0, np.abs(lw_r)))
    z_g, z_r = got["z"][dec], ref["z"][dec]
    assert np.all(np.abs(z_g - z_r) <= TOL * np.maximum(1.0, np.abs(z_r)))
    if len(case) == 9:
        assert 0.0 < rate < 1.0          # both branches of the accept test ran


# --------------------------------------------------------------------------------------------------------- 2. bit-equalities
def _bits_case():
    d = O.Dims(D=23, L=5, K=3, hidden=(12, 20), act="relu")
    model = O.MODEL_GMVAE
    p, flat, x = make(model, d, 4, 77)
    base = tuple(a.astype(np.float32) for a in R.encoder_table(model, d, p, x))
    return model, d, flat, x, base, R.schedule("sigmoid", 8).astype(np.float32)


def _same(a, b):
    for k in ("logw", "bound", "stats", "z", "tail", "bits"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("init", ["prior", "encoder"])
def test_bit_equalities(init, monkeypatch):
    monkeypatch.delenv("GMVAE_AIS_LAUNCH_TEMPS", raising=False)
    model, d, flat, x, base, betas = _bits_case()
    base = base if init == "encoder" else None
    C_ = 5                                 # 20 chains: a full panel and a ragged one; 10 per half: one ragged panel
    one = device_ais(model, d, flat, x, betas, C_, 3, 0.5, base)
    # two identical calls
    _same(one, device_ais(model, d, flat, x, betas, C_, 3, 0.5, base))
    # in-kernel Philox against the same draws supplied as arrays
    eps, u = device_noise(8, 4 * C_, d.L, 0, 7, 3)
    _same(one, device_ais(model, d, flat, x, betas, C_, 3, 0.5, base, eps, u))
    # T = 8 in one launch against launches of 3 + 3 + 2 transitions
    monkeypatch.setenv("GMVAE_AIS_LAUNCH_TEMPS", "3")
    _same(one, device_ais(model, d, flat, x, betas, C_, 3, 0.5, base))
    monkeypatch.delenv("GMVAE_AIS_LAUNCH_TEMPS")
    # B = 4 in one call against two calls of B = 2, the second at row0 = 2
    halves = [device_ais(model, d, flat, x[h:h + 2], betas, C_, 3, 0.5, None if base is None else tuple(a[h:h + 2] for a in base),
                         row0=h) for h in (0, 2)]
    for k in ("logw", "bound", "stats", "z", "bits"):
        assert np.array_equal(np.concatenate([h[k] for h in halves]).view(np.uint8), one[k].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------------- 3. existing code
@pytest.mark.parametrize("name", ["vae", "vae_gmp"])
def test_one_temperature_from_the_encoder_is_the_forward_and_the_iw_bound(name):
    """T = 1, init="encoder", step 0: log w is Engine.forward(n_samples=C)'s row log w, the bound is iw_bound(x, C)."""
    from gmvae_amd.engine import Engine
    C_, B = 6, 5
    e = Engine(name, 23, 5, 1 if name == "vae" else 4, [12, 20], random_seed=3)
    rng = np.random.default_rng(9)
    with torch.no_grad():
        e.params.mul_(2.0)
    x = torch.from_numpy((rng.random((B, 23)) < 0.5).astype(np.uint8)).cuda()
    assert e.global_step == 0
    a = e.ais_bound(x, n_chains=C_, n_temps=1, init="encoder", n_leapfrog=2, step_size=0.3)
    f = e.forward(x, n_samples=C_)
    lw = f["rows"][:, 3].reshape(B, C_).double()
    assert torch.all((a["logw"].double() - lw).abs() <= TOL * lw.abs().clamp_min(1.0))
    ib = e.iw_bound(x, C_)["bound"].double()
    assert torch.all((a["bound"].double() - ib).abs() <= TOL * ib.abs().clamp_min(1.0))


# ------------------------------------------------------------------------------------------- 4. quadrature; stats and tail
def test_quadrature_on_the_device():
    """The CPU test's L = 2 GMVAE with in-kernel noise: every example's bound within 4 standard errors of the trapezoid value."""
    d = O.Dims(D=24, L=2, K=3, hidden=(16,), act="tanh")
    model = O.MODEL_GMVAE
    p, flat, x = make(model, d, 4, 5)
    q = R.quadrature_log_px(model, d, p, x)
    got = device_ais(model, d, flat, x, R.schedule("sigmoid", 256).astype(np.float32), 64, 5, 0.3)
    se = R.bound_stderr(got["logw"])
    print(f"err {got['bound'] - q}, se {se}, accept {got['stats'][:, 2]}")
    assert np.all(np.abs(got["bound"] - q) <= 4 * se)


def test_stats_and_tail_against_their_definitions():
    model, d, flat, x, base, betas = _bits_case()
    C_, T = 5, 8
    got = device_ais(model, d, flat, x, betas, C_, 3, 0.5, base)
    lw = got["logw"].astype(np.float64)
    m = lw.max(axis=1, keepdims=True)
    w = np.exp(lw - m)
    bound = m[:, 0] + np.log(w.sum(axis=1)) - math.log(C_)
    ess = w.sum(axis=1) ** 2 / (w * w).sum(axis=1)
    acc = accept_matrix(got["bits"], T)
    rate = acc.reshape(T, 4, C_).mean(axis=(0, 2))
    step = (0.5 * 1.02 ** acc.sum(axis=0) * 0.96 ** (T - acc.sum(axis=0))).reshape(4, C_).mean(axis=1)      # (no clip reached)
    want = np.stack([bound, ess, rate, step], axis=1)
    np.testing.assert_allclose(got["bound"], bound, rtol=2e-6, atol=2e-6)      # log w was rounded to fp32 on the way out
    np.testing.assert_allclose(got["stats"], want, rtol=2e-5, atol=2e-6)
    tail = np.array([-got["stats"][:, 0].astype(np.float64).sum(), *got["stats"][:, 1:].astype(np.float64).sum(axis=0), 4, 0, 0, 0])
    np.testing.assert_allclose(got["tail"], tail, rtol=1e-6, atol=1e-6)
    assert np.all((ess >= 1 - 1e-9) & (ess <= C_ + 1e-9))


def test_model_surface_and_adaptation_switch():
    """model.ais_bound on the three models; adapt=False keeps every chain's step size; the GMVAE's bound sits ln K below
    iw_bound_enum_y's convention, so it is compared as bound + ln K."""
    from gmvae_amd.engine import ais_schedule
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(2)
    x = torch.from_numpy((rng.random((6, 24)) < 0.5).astype(np.uint8)).cuda()
    for K in (1, 3):
        r = create_vae(24, 3, mixture_components=K, fcnet_hidden_sizes=[16], random_seed=1).ais_bound(x, 4, 8, n_leapfrog=2)
        assert r["bound"].shape == (6,) and bool(torch.isfinite(r["bound"]).all())
    model = create_gmvae(24, 3, mixture_components=4, fcnet_hidden_sizes=[16], random_seed=1)
    assert torch.equal(model.ais_bound(x, 4, 8, n_leapfrog=2)["bound"], model._engine.ais_bound(x, 4, 8, n_leapfrog=2)["bound"])
    e = model._engine
    a = e.ais_bound(x, n_chains=8, n_temps=64, n_leapfrog=4, step_size=0.2, adapt=False)
    assert torch.all(a["stats"][:, 3] == torch.tensor(0.2, dtype=torch.float32))
    assert a["z"].shape == (48, 3) and a["logw"].shape == (6, 8) and float(a["tail"][4]) == 6
    enum = e.iw_bound_enum_y(x, 512)["bound"]
    assert torch.all((a["bound"] + math.log(4) - enum).abs() < 0.5)      # an untrained, near-linear model: both near log p(x) + ln K
    b = e.ais_bound(x, n_chains=8, n_temps=64, n_leapfrog=4, step_size=0.2, adapt=False, schedule=ais_schedule("sigmoid", 64))
    assert torch.equal(a["logw"], b["logw"])
    with pytest.raises(ValueError):
        e.ais_bound(x, schedule=torch.linspace(0, 1, 5), n_temps=8)
    with pytest.raises(ValueError):
        e.ais_bound(x, init="posterior")


def test_run_eval_reports_the_ais_estimate(tmp_path):
    """run_gmvae --mode=eval --ais_chains C --ais_temps T: ais_log_px, the chains' ESS and acceptance rate, and the gap to the
    y-summed-out importance-weighted bound (its ln K put back), over the whole split and independent of --batch_size."""
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=128", "--max_steps=20", "--summarise_every=20", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=256"]
    run_gmvae.main(["--mode=train"] + args)
    ais = ["--ais_chains=4", "--ais_temps=16", "--ais_leapfrog=3", "--iw_enum_samples=16"]
    res = run_gmvae.main(["--mode=eval"] + args + ais)
    assert res["examples"] == 256 and res["ais_stats"].shape == (256, 4)
    assert res["train/ais_log_px"] == pytest.approx(res["ais_stats"][:, 0].double().mean().item(), rel=1e-9)
    assert 1.0 <= res["train/ais_ess"] <= 4.0 and 0.0 < res["train/ais_accept_rate"] <= 1.0
    gap = res["train/ais_log_px"] + math.log(10) - res["train/iw_bound_enum_y_16_per_example"]
    assert res["train/ais_gap_to_iw_bound_enum_y"] == pytest.approx(gap, abs=1e-6)
    assert -600.0 < res["train/ais_log_px"] < -100.0          # Bernoulli(0.87) pixels: about -784 * 0.386 = -303 at best
    other = run_gmvae.main(["--mode=eval"] + [a if not a.startswith("--batch_size") else "--batch_size=64" for a in args] + ais)
    assert torch.equal(other["ais_stats"], res["ais_stats"])


@pytest.mark.parametrize("init", ["prior", "encoder"])
def test_memory_contract_on_guarded_buffers(init):
    """gmvae_ais on arena buffers at their exact sizes (23 pixels, L = 5, 3 x 5 chains: a ragged panel that spans examples; the
    workspace at exactly the bytes its size query answers, 0xFF-filled): nothing changes but the outputs and the workspace, with
    every optional output present and with all of them NULL, and the results are those of the plain call."""
    from arena import Arena
    L = _L()
    model, d, flat, x, base, betas = _bits_case()
    x, C_, T = x[:3], 5, 8
    B, n = 3, 15
    base = tuple(a[:3] for a in base) if init == "encoder" else None
    want = device_ais(model, d, flat, x, betas, C_, 3, 0.5, base)
    cd = dims_of(d, B)
    base_K = 0 if base is None else base[0].shape[1]
    ar = Arena("cuda", 4 << 20)
    f32 = torch.float32
    ins = {"params": (flat, f32, 4 * 23), "x": (x, torch.uint8, 23), "betas": (betas, f32, 4 * (T + 1))}
    if base is not None:
        ins["base"] = (np.concatenate([a.reshape(B, -1) for a in base], axis=1), f32, 4 * base_K * (1 + 2 * d.L))
    bufs = {}
    for name, (a, dt, pitch) in ins.items():
        t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dt)
        bufs[name] = ar.place(name, t.numel() * t.element_size(), pitch, False, dt)
        bufs[name].copy_(t)
    outs = {"logw": (n, 4 * C_), "bound": (B, 4), "stats": (4 * B, 16), "z": (n * d.L, 4 * d.L), "tail": (L.TAIL, 4 * L.TAIL)}
    for name, (count, pitch) in outs.items():
        bufs[name] = ar.place(name, 4 * count, pitch, True, f32)
    ws = ar.place("workspace", L.ais_workspace_bytes(cd, model, base_K, C_), 4 * d.L, True, torch.uint8)
    for with_outputs in (True, False):
        for name in ("logw", "bound", "stats", "z"):
            ar.set_writable(name, with_outputs)
            bufs[name].fill_(float("nan"))
        ws.fill_(0xFF)
        o = (lambda k: L.ptr(bufs[k])) if with_outputs else (lambda k: None)
        ar.snapshot()
        rc = L.lib.gmvae_ais(C.byref(cd), model, L.ptr(bufs["x"]), L.ptr(bufs["params"]), L.ptr(bufs.get("base")), base_K,
                             L.ptr(bufs["betas"]), T, C_, 3, 0.5, 1.02, 0.96, None, None, o("logw"), o("bound"), o("stats"), o("z"),
                             L.ptr(bufs["tail"]), L.ptr(ws), 7, 3, L.current_stream())
        L.check(rc, "gmvae_ais")
        ar.check()
        assert np.array_equal(bufs["tail"].cpu().numpy().view(np.uint8), want["tail"].view(np.uint8))
        if with_outputs:
            for k in ("logw", "bound", "stats", "z"):
                assert np.array_equal(bufs[k].cpu().numpy().view(np.uint8), want[k].reshape(-1).view(np.uint8)), k
