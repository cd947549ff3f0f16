"""gmvae_simulate and gmvae_ais_reverse (include/gmvae_hip.h; csrc/bdmc.hpp) on the device against the fp64 statement
(tests/bdmc_ref.py): parity of the simulation and of the reverse chains on the device's own noise over the three models, both
bases, the activations, ragged sizes and the size gates' corners (tests/bdmc_cases.py; their conditions are held on the CPU by
tests/test_bdmc_cpu.py); bit-equalities of both entry points (in-kernel Philox against supplied noise, the batch split, the launch
cut, two calls, bdmc_gap's forward half against ais_bound); the sandwich around quadrature on a two-dimensional latent; stats and
tail; the memory contract on guarded buffers; the Python surface.

Parity of the chains holds the statement's DECIDED chains to the accept sequence exactly and to 1e-4 max(1, |.|) in log w_rev and
z_0 -- the project's gate, as tests/test_ais.py --; of the simulation, z* to the same gate, k exactly, x exactly on every pixel
whose uniform is not within 1e-5 of its threshold, prob to 1e-4."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ais_ref as A
import bdmc_cases as K
import bdmc_ref as R
import oracle as O
from hip_util import dev, dims_of
from test_ais import accept_matrix, device_ais, device_noise

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _L():
    from gmvae_amd import _lib
    return _lib


def device_sim_noise(B, d, row0=0, seed=K.SEED, step=K.STEP):
    """The draws gmvae_simulate makes itself, as arrays: eps [B, L], u [B] (gmvae_noise_fill at step 2 step), ux [B, D] (the u of
    a one-column fill at 2 step + 1)."""
    L = _L()
    f32 = dict(dtype=torch.float32, device="cuda")
    e, u, ux = torch.empty(B, d.L, **f32), torch.empty(B, 1, **f32), torch.empty(B, d.D, **f32)
    L.check(L.lib.gmvae_noise_fill(L.ptr(e), L.ptr(u), B, d.L, 1, row0, seed, 2 * step, None, L.current_stream()), "gmvae_noise_fill")
    L.check(L.lib.gmvae_noise_fill(None, L.ptr(ux), B, 1, d.D, row0, seed, 2 * step + 1, None, L.current_stream()), "gmvae_noise_fill")
    return e, u.reshape(B), ux


def device_sim(model, d, flat, B, eps=None, u=None, ux=None, row0=0, seed=K.SEED, step=K.STEP, prob=True):
    """One gmvae_simulate call on fresh buffers: dict of numpy outputs."""
    L = _L()
    cd = dims_of(d, B)
    cd.row0 = row0
    ws = torch.full((L.simulate_workspace_bytes(cd, model) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    o = dict(z=torch.empty(B, d.L, dtype=torch.float32, device="cuda"), k=torch.empty(B, dtype=torch.int32, device="cuda"),
             x=torch.empty(B, d.D, dtype=torch.uint8, device="cuda"), prob=torch.empty(B, d.D, dtype=torch.float32, device="cuda"))
    fl = dev(flat)
    rc = L.lib.gmvae_simulate(C.byref(cd), model, L.ptr(fl), L.ptr(eps), L.ptr(u), L.ptr(ux), L.ptr(o["z"]), L.ptr(o["k"]),
                              L.ptr(o["x"]), L.ptr(o["prob"]) if prob else None, L.ptr(ws), seed, step, L.current_stream())
    L.check(rc, "gmvae_simulate")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items() if prob or k != "prob"}


def device_rev(model, d, flat, x, z_start, betas, C_, n_leap, step0, base=None, eps=None, u=None, row0=0, seed=K.SEED,
               step=K.STEP_REV, up=1.02, down=0.96):
    """One gmvae_ais_reverse call on fresh buffers: dict of numpy outputs and the accept records [B C] (uint64)."""
    L = _L()
    B = x.shape[0]
    cd = dims_of(d, B)
    cd.row0 = row0
    n, T = B * C_, len(betas) - 1
    base_K = 0 if base is None else base[0].shape[1]
    bd = None
    if base is not None:
        bd = dev(np.concatenate([np.asarray(a, np.float32).reshape(B, -1) for a in base], axis=1))
    nbytes = L.ais_reverse_workspace_bytes(cd, model, base_K, C_)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")      # (needs no initialisation)
    f32 = dict(dtype=torch.float32, device="cuda")
    o = dict(logw=torch.empty(B, C_, **f32), bound=torch.empty(B, **f32), stats=torch.empty(B, 4, **f32),
             z=torch.empty(n, d.L, **f32), tail=torch.empty(L.TAIL, **f32))
    keep = (dev(flat), dev(x), dev(np.asarray(betas, np.float32)), dev(np.asarray(z_start, np.float32)))
    rc = L.lib.gmvae_ais_reverse(C.byref(cd), model, L.ptr(keep[1]), L.ptr(keep[0]), L.ptr(bd), base_K, L.ptr(keep[3]),
                                 L.ptr(keep[2]), T, C_, n_leap, step0, up, down, L.ptr(eps), L.ptr(u), L.ptr(o["logw"]),
                                 L.ptr(o["bound"]), L.ptr(o["stats"]), L.ptr(o["z"]), L.ptr(o["tail"]), L.ptr(ws), seed, step,
                                 L.current_stream())
    L.check(rc, "gmvae_ais_reverse")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["bits"] = ws[:2 * n].cpu().numpy().view(np.uint64)
    return out


# ----------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", K.CASES, ids=K.cid)
def test_parity_against_the_statement(case):
    """The simulation on the device's own draws, then the reverse chains from the DEVICE's (x, z*) on the device's own draws."""
    model, d, init, B, C_, T, leap, explicit = K.unpack_case(case)
    p, flat = K.case_model(case)
    # ---- the simulation
    e, u, ux = device_sim_noise(B, d)
    sim = device_sim(model, d, flat, B, e, u, ux)
    ref = R.simulate(model, d, p, e.cpu().numpy(), u.cpu().numpy(), ux.cpu().numpy())
    clear = ref["pix_margin"] > 1e-5
    print(f"{K.cid(case)}: simulation: pixels in the band {int((~clear).sum())} of {clear.size}, nearest CDF edge {ref['edge'].min():.2e}, "
          f"max |dz| {np.abs(sim['z'] - ref['z']).max():.2e}, max |dprob| {np.abs(sim['prob'] - ref['prob']).max():.2e}")
    assert (~clear).mean() <= 0.01 and ref["edge"].min() > 1e-6
    assert np.array_equal(sim["k"], ref["k"])
    assert np.all(np.abs(sim["z"] - ref["z"]) <= TOL * np.maximum(1.0, np.abs(ref["z"])))
    assert np.array_equal(sim["x"][clear], ref["x"][clear]) and set(np.unique(sim["x"])) <= {0, 1}
    assert np.all(np.abs(sim["prob"] - ref["prob"]) <= TOL)
    # ---- the reverse chains
    x, z = sim["x"], sim["z"]
    betas = R.schedule("sigmoid", T).astype(np.float32)
    base = tuple(a.astype(np.float32) for a in A.encoder_table(model, d, p, x)) if init == "encoder" else None
    eps, uu = device_noise(T, B * C_, d.L, 0, K.SEED, K.STEP_REV)
    got = device_rev(model, d, flat, x, z, betas, C_, leap, K.STEP0, base, eps, uu)
    want = R.reverse_ais(model, d, p, x, z.astype(np.float64), betas.astype(np.float64), C_, leap, K.STEP0, eps.cpu().numpy(),
                         uu.cpu().numpy(), init, base=base)
    dec = want["decided"]
    acc = accept_matrix(got["bits"], T)
    rate = want["accepts"].mean()
    print(f"{K.cid(case)}: chains: undecided {int((~dec).sum())} of {dec.size}, accept rate {rate:.2f}, "
          f"max |dlogw| {np.abs(got['logw'].reshape(-1) - want['logw'].reshape(-1))[dec].max(initial=0):.2e}")
    assert (~dec).mean() <= 0.10
    assert np.array_equal(acc[:, dec], want["accepts"][:, dec])
    lw_g, lw_r = got["logw"].reshape(-1)[dec], want["logw"].reshape(-1)[dec]
    assert np.all(np.abs(lw_g - lw_r) <= TOL * np.maximum(1.0, np.abs(lw_r)))
    z_g, z_r = got["z"][dec], want["z"][dec]
    assert np.all(np.abs(z_g - z_r) <= TOL * np.maximum(1.0, np.abs(z_r)))
    if not explicit:
        assert 0.0 < rate < 1.0          # both branches of the accept test ran


# --------------------------------------------------------------------------------------------------------- 2. bit-equalities
def _bits_case():
    d = O.Dims(D=23, L=5, K=3, hidden=(12, 20), act="relu", gen_bias_init=np.linspace(-0.5, 0.5, 23).astype(np.float32))
    model = O.MODEL_GMVAE
    p, flat = K.make(model, d, 77)
    sim = device_sim(model, d, flat, 4)
    base = tuple(a.astype(np.float32) for a in A.encoder_table(model, d, p, sim["x"]))
    return model, d, flat, sim, base, R.schedule("sigmoid", 8).astype(np.float32)


def _same(a, b, keys=("logw", "bound", "stats", "z", "tail", "bits")):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("init", ["prior", "encoder"])
def test_bit_equalities_of_the_reverse_chains(init, monkeypatch):
    monkeypatch.delenv("GMVAE_AIS_LAUNCH_TEMPS", raising=False)
    model, d, flat, sim, base, betas = _bits_case()
    base = base if init == "encoder" else None
    x, z = sim["x"], sim["z"]
    C_ = 5                                 # 20 chains: a full panel and a ragged one; 10 per half: one ragged panel
    one = device_rev(model, d, flat, x, z, betas, C_, 3, 0.5, base)
    assert one["bits"].any()
    # two identical calls
    _same(one, device_rev(model, d, flat, x, z, betas, C_, 3, 0.5, base))
    # in-kernel Philox against the same draws supplied as arrays (slot 0 is never read: NaN there)
    eps, u = device_noise(8, 4 * C_, d.L, 0, K.SEED, K.STEP_REV)
    eps[0], u[0] = float("nan"), float("nan")
    _same(one, device_rev(model, d, flat, x, z, betas, C_, 3, 0.5, base, eps, u))
    # T = 8 in one launch against launches of 3 + 3 + 2 transitions, descending
    monkeypatch.setenv("GMVAE_AIS_LAUNCH_TEMPS", "3")
    _same(one, device_rev(model, d, flat, x, z, betas, C_, 3, 0.5, base))
    monkeypatch.delenv("GMVAE_AIS_LAUNCH_TEMPS")
    # B = 4 in one call against two calls of B = 2, the second at row0 = 2
    halves = [device_rev(model, d, flat, x[h:h + 2], z[h:h + 2], betas, C_, 3, 0.5,
                         None if base is None else tuple(a[h:h + 2] for a in base), row0=h) for h in (0, 2)]
    for k in ("logw", "bound", "stats", "z", "bits"):
        assert np.array_equal(np.concatenate([h[k] for h in halves]).view(np.uint8), one[k].view(np.uint8)), k


def test_bit_equalities_of_the_simulation():
    """D = 23 with two hidden layers, 20 examples: a full panel and a ragged one."""
    d = O.Dims(D=23, L=5, K=3, hidden=(12, 20), act="relu", gen_bias_init=np.linspace(-0.5, 0.5, 23).astype(np.float32))
    model = O.MODEL_VAE_GMP
    _, flat = K.make(model, d, 78)
    B = 20
    keys = ("z", "k", "x", "prob")
    one = device_sim(model, d, flat, B)
    assert 0 < one["x"].mean() < 1 and len(np.unique(one["k"])) > 1
    _same(one, device_sim(model, d, flat, B), keys)
    _same(one, device_sim(model, d, flat, B, *device_sim_noise(B, d)), keys)
    halves = [device_sim(model, d, flat, n, row0=r) for r, n in ((0, 7), (7, 13))]
    for k in keys:
        assert np.array_equal(np.concatenate([h[k] for h in halves]).view(np.uint8), one[k].view(np.uint8)), k
    _same(one, device_sim(model, d, flat, B, prob=False), ("z", "k", "x"))
    other = device_sim(model, d, flat, B, step=K.STEP + 1)
    assert not np.array_equal(other["z"], one["z"]) and not np.array_equal(other["x"], one["x"])


# ------------------------------------------------------------------------------------------- 3. quadrature; stats and tail
def test_quadrature_on_the_device():
    """The L = 2 GMVAE of the CPU tests, 4 examples simulated on the device, in-kernel noise, T = 256, C = 64: lower <= quadrature
    <= upper within 4 standard errors each."""
    d = O.Dims(D=24, L=2, K=3, hidden=(16,), act="tanh")
    model = O.MODEL_GMVAE
    p, flat = K.make(model, d, 5)
    sim = device_sim(model, d, flat, 4)
    q = A.quadrature_log_px(model, d, p, sim["x"])
    betas = R.schedule("sigmoid", 256).astype(np.float32)
    lo = device_ais(model, d, flat, sim["x"], betas, 64, 5, 0.3)
    up = device_rev(model, d, flat, sim["x"], sim["z"], betas, 64, 5, 0.3)
    se_lo, se_up = R.bound_stderr(lo["logw"]), R.bound_stderr(up["logw"])
    print(f"lower - quad {lo['bound'] - q}, se {se_lo}; upper - quad {up['bound'] - q}, se {se_up}; accept {up['stats'][:, 2]}")
    assert np.all(lo["bound"] - q <= 4 * se_lo) and np.all(q - up["bound"] <= 4 * se_up)
    assert np.all(np.abs(lo["bound"] - q) <= 4 * se_lo) and np.all(np.abs(up["bound"] - q) <= 4 * se_up)


def test_stats_and_tail_against_their_definitions():
    model, d, flat, sim, base, betas = _bits_case()
    C_, T = 5, 8
    got = device_rev(model, d, flat, sim["x"], sim["z"], betas, C_, 3, 0.5, base)
    lw = got["logw"].astype(np.float64)
    m = lw.max(axis=1, keepdims=True)
    w = np.exp(lw - m)
    bound = -(m[:, 0] + np.log(w.sum(axis=1)) - math.log(C_))
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


# ------------------------------------------------------------------------------------------------------- 4. memory contract
@pytest.mark.parametrize("init", ["prior", "encoder"])
def test_memory_contract_of_the_reverse_chains(init):
    """gmvae_ais_reverse on arena buffers at their exact sizes (23 pixels, L = 5, 3 x 5 chains; the workspace at exactly the bytes
    its size query answers, 0xFF-filled): nothing changes but the outputs and the workspace, with every optional output present and
    with all of them NULL, and the results are those of the plain call."""
    from arena import Arena
    L = _L()
    model, d, flat, sim, base, betas = _bits_case()
    x, z, C_, T = sim["x"][:3], sim["z"][:3], 5, 8
    B, n = 3, 15
    base = tuple(a[:3] for a in base) if init == "encoder" else None
    want = device_rev(model, d, flat, x, z, betas, C_, 3, 0.5, base)
    base_K = 0 if base is None else base[0].shape[1]
    ar = Arena("cuda", 4 << 20)
    f32 = torch.float32
    cd = dims_of(d, B, ar)                     # (the bias vector sits in the arena too)
    ins = {"params": (flat, f32, 4 * 23), "x": (x, torch.uint8, 23), "betas": (betas, f32, 4 * (T + 1)), "z_start": (z, f32, 4 * d.L)}
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
    ws = ar.place("workspace", L.ais_reverse_workspace_bytes(cd, model, base_K, C_), 4 * d.L, True, torch.uint8)
    for with_outputs in (True, False):
        for name in ("logw", "bound", "stats", "z"):
            ar.set_writable(name, with_outputs)
            bufs[name].fill_(float("nan"))
        ws.fill_(0xFF)
        o = (lambda k: L.ptr(bufs[k])) if with_outputs else (lambda k: None)
        ar.snapshot()
        rc = L.lib.gmvae_ais_reverse(C.byref(cd), model, L.ptr(bufs["x"]), L.ptr(bufs["params"]), L.ptr(bufs.get("base")), base_K,
                                     L.ptr(bufs["z_start"]), L.ptr(bufs["betas"]), T, C_, 3, 0.5, 1.02, 0.96, None, None, o("logw"),
                                     o("bound"), o("stats"), o("z"), L.ptr(bufs["tail"]), L.ptr(ws), K.SEED, K.STEP_REV,
                                     L.current_stream())
        L.check(rc, "gmvae_ais_reverse")
        ar.check()
        assert np.array_equal(bufs["tail"].cpu().numpy().view(np.uint8), want["tail"].view(np.uint8))
        if with_outputs:
            for k in ("logw", "bound", "stats", "z"):
                assert np.array_equal(bufs[k].cpu().numpy().view(np.uint8), want[k].reshape(-1).view(np.uint8)), k


def test_memory_contract_of_the_simulation():
    """gmvae_simulate on arena buffers at their exact sizes (23 pixels, 19 examples: a ragged second panel; hidden (12, 20)), with
    prob_out and without: nothing changes but the outputs and the workspace, and the results are those of the plain call."""
    from arena import Arena
    L = _L()
    d = O.Dims(D=23, L=5, K=3, hidden=(12, 20), act="relu", gen_bias_init=np.linspace(-0.5, 0.5, 23).astype(np.float32))
    model = O.MODEL_GMVAE
    _, flat = K.make(model, d, 79)
    B = 19
    want = device_sim(model, d, flat, B)
    ar = Arena("cuda", 4 << 20)
    f32 = torch.float32
    cd = dims_of(d, B, ar)                     # (the bias vector sits in the arena too)
    params = ar.place("params", 4 * flat.size, 4 * 23, False, f32)
    params.copy_(torch.from_numpy(flat))
    bufs = {"z": ar.place("z", 4 * B * d.L, 4 * d.L, True, f32), "k": ar.place("k", 4 * B, 4, True, torch.int32),
            "x": ar.place("x", B * d.D, d.D, True, torch.uint8), "prob": ar.place("prob", 4 * B * d.D, 4 * d.D, True, f32)}
    ws = ar.place("workspace", L.simulate_workspace_bytes(cd, model), 4 * d.L, True, torch.uint8)
    for with_prob in (True, False):
        ar.set_writable("prob", with_prob)
        for b in bufs.values():
            b.fill_(0x7F if b.dtype != f32 else float("nan"))
        ws.fill_(0xFF)
        ar.snapshot()
        rc = L.lib.gmvae_simulate(C.byref(cd), model, L.ptr(params), None, None, None, L.ptr(bufs["z"]), L.ptr(bufs["k"]),
                                  L.ptr(bufs["x"]), L.ptr(bufs["prob"]) if with_prob else None, L.ptr(ws), K.SEED, K.STEP,
                                  L.current_stream())
        L.check(rc, "gmvae_simulate")
        ar.check()
        for k in ("z", "k", "x") + (("prob",) if with_prob else ()):
            assert np.array_equal(bufs[k].cpu().numpy().view(np.uint8), want[k].reshape(-1).view(np.uint8)), k


# --------------------------------------------------------------------------------------------------------------- 5. surface
def test_model_surface_and_the_forward_half():
    """model.simulate / model.bdmc_gap on the three models; bdmc_gap's forward half is ais_bound on the simulated x, bit for bit;
    the three Philox keys are disjoint; adapt=False keeps every chain's step size in both directions."""
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    models = [create_vae(24, 3, mixture_components=K_, fcnet_hidden_sizes=[16], random_seed=1) for K_ in (1, 3)]
    models.append(create_gmvae(24, 3, mixture_components=4, fcnet_hidden_sizes=[16], random_seed=1))
    for m in models:
        with torch.no_grad():
            m._engine.params.mul_(2.0)
        s = m.simulate(6)
        assert s["z"].shape == (6, 3) and s["k"].shape == (6,) and s["x"].shape == (6, 24) and s["prob"].shape == (6, 24)
        assert s["x"].dtype == torch.uint8 and s["k"].dtype == torch.int32 and int(s["x"].max()) <= 1
        assert bool(((s["k"] >= 0) & (s["k"] < m._engine.K if m._engine.model else s["k"] == 0)).all())
        g = m.bdmc_gap(6, 4, 8, n_leapfrog=2, step_size=0.2)
        assert torch.equal(g["x"], s["x"]) and torch.equal(g["z"], s["z"]) and torch.equal(g["k"], s["k"])
        a = m.ais_bound(g["x"], 4, 8, n_leapfrog=2, step_size=0.2)
        for k in ("bound", "logw", "stats", "z", "tail"):
            assert torch.equal(g["forward"][k], a[k]), k
        assert torch.equal(g["lower"], a["bound"]) and g["upper"].shape == (6,) and bool(torch.isfinite(g["upper"]).all())
        assert torch.equal(g["gap"], g["upper"].double() - g["lower"].double())
        assert g["gap_mean"] == pytest.approx(g["upper_mean"] - g["lower_mean"], abs=1e-9)
        assert bool(((g["upper_ess"] >= 1 - 1e-5) & (g["upper_ess"] <= 4 + 1e-5)).all())
        # the reverse chains do not reuse the forward chains' draws: with the forward key they give other bits
        e = m._engine
        same_key = e._ais_chains("ais_bound_reverse", g["x"], g["z"], 4, 8, "sigmoid", 2, 0.2, "prior", True, None, None, None, 1.02,
                                 0.96, e.noise_seed)
        assert not torch.equal(same_key["logw"], g["reverse"]["logw"])
        assert torch.equal(e.ais_bound_reverse(g["x"], g["z"], 4, 8, n_leapfrog=2, step_size=0.2)["logw"], g["reverse"]["logw"])
        f = m.bdmc_gap(6, 4, 8, n_leapfrog=2, step_size=0.2, adapt=False, init="encoder")
        for half in ("forward", "reverse"):
            assert torch.all(f[half]["stats"][:, 3] == torch.tensor(0.2, dtype=torch.float32))
    with pytest.raises(ValueError):
        models[0]._engine.ais_bound_reverse(s["x"], s["z"][:, :2], 4, 8)
    with pytest.raises(ValueError):
        models[0].simulate(0)


def test_run_eval_reports_the_bdmc_figures(tmp_path):
    """run_gmvae --mode=eval --bdmc_examples N at the --ais_* settings: the five figures, over N simulated examples whatever
    --batch_size, and a second run gives the same bits."""
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=128", "--max_steps=20", "--summarise_every=20", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=256"]
    run_gmvae.main(["--mode=train"] + args)
    bd = ["--ais_chains=4", "--ais_temps=16", "--ais_leapfrog=3", "--bdmc_examples=48"]
    res = run_gmvae.main(["--mode=eval"] + args + bd)
    st = res["bdmc_stats"]
    assert st.shape == (48, 4)
    assert res["train/bdmc_lower"] == pytest.approx(st[:, 0].double().mean().item(), rel=1e-9)
    assert res["train/bdmc_upper"] == pytest.approx(st[:, 1].double().mean().item(), rel=1e-9)
    assert res["train/bdmc_gap"] == pytest.approx(res["train/bdmc_upper"] - res["train/bdmc_lower"], abs=1e-9)
    assert 1.0 <= res["train/bdmc_reverse_ess"] <= 4.0 and 0.0 < res["train/bdmc_reverse_accept_rate"] <= 1.0
    assert -600.0 < res["train/bdmc_lower"] < -100.0 and res["train/bdmc_gap"] > 0.0      # 16 temperatures from the prior: far apart
    again = run_gmvae.main(["--mode=eval"] + args + bd)
    assert torch.equal(again["bdmc_stats"], st)
    other = run_gmvae.main(["--mode=eval"] + [a if not a.startswith("--batch_size") else "--batch_size=32" for a in args] + bd)
    assert torch.equal(other["bdmc_stats"], st)
