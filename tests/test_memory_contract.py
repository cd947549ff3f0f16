"""-m gpu: every entry point held to the bytes its caller owns (include/gmvae_hip.h says which those are).

Every device buffer of a call lies in a guarded arena (tests/arena.py; tests/test_memory_contract_cpu.py holds the arena itself
to what it must report): exact-size buffers, 0xFF everywhere, the workspace at exactly the bytes its size query answers, zeroed.
After the call every byte outside the call's writable set -- the guard bands around each buffer, and x, eps, u, params, idx and
the caller-written workspace regions, which the library only reads -- must be bit-identical to a snapshot taken just before it.

  A  gmvae_step at every `step` corner of tests/gate_corners.py, through compare_step(alloc=arena): the fp64 gates AND the guards;
     one corner per schedule word again with in-kernel noise and a device step counter
  B  gmvae_forward at the evalf corners and one corner per schedule word: all four optional outputs, then each alone
  C  3-step train graphs through the C ABI at every `train` corner, bit for bit the same graph in plain allocations; batches at
     4-byte-aligned and odd addresses against 1-step graphs on aligned batches
  D  one gmvae_step and one gmvae_forward per legal set of objective / optimizer bits at a shape where nothing is a multiple of
     4 or 16, all 32 slots of every caller-written region filled and read-only, bit for bit the plain call; the same under every
     set of likelihood bits, x as bytes or as floats at exactly its size, D = 100 and 99
  E  the chunked evaluators (bit for bit the plain call) and the small entry points (their existing CPU restatements)

A NaN or a 255 that leaks in from a guard band cannot pass the oracle gates of A and B; C, D and E compare paths the header
documents as free of atomics with the same call in plain allocations.  profiles/memory_contract_notes.md has the figures."""
import ctypes as C
import dataclasses
import math
import time

import numpy as np
import pytest
import torch

import arena as A
import gate_corners as G
import oracle as O
from test_step_inputs_cpu import CONSTRUCTIONS

pytestmark = pytest.mark.gpu

CAPACITY = 1 << 29
STATS = {}              # group -> [cases, largest arena in bytes, seconds between the first placement and the last check]


@pytest.fixture(scope="module")
def H():
    import hip_util
    return hip_util


@pytest.fixture(scope="module")
def L():
    from gmvae_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def arena():
    return A.Arena("cuda", CAPACITY)


class _Timed:
    """Counts one case of `group`: the arena's size at the end and the wall time, host work (the fp64 oracle) included."""

    def __init__(self, group, arena):
        self.group, self.arena = group, arena

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        s = STATS.setdefault(self.group, [0, 0, 0.0])
        s[0] += 1
        s[1] = max(s[1], self.arena.used)
        s[2] += time.perf_counter() - self.t0


def _set_env(monkeypatch, c):
    for k in G.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _of_kind(kind):
    cs = [c for c in G.CORNERS if c.kind == kind]
    return pytest.mark.parametrize("c", cs, ids=[c.id for c in cs])


def _corner_inputs(c, B):
    """test_step_at_gate_corner_matches_oracle's preparation."""
    model, d = O.MODEL_NAMES[c.model], c.d
    rng = np.random.default_rng(B)
    p = O.init_params(model, d, rng)
    for k in p:
        if k.endswith("/b"):
            p[k] = rng.normal(0, 0.05, p[k].shape)
    x, eps, u = O.make_inputs(d, B, model)
    return model, d, p, x, eps, u


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{what}: {bad.size} bytes differ between the arena and the plain call, first at byte {bad[0]}"


# ------------------------------------------------------------------------------------- the arena itself, on the device
def test_arena_reports_on_the_device(L, arena):
    """What tests/test_memory_contract_cpu.py shows on the CPU holds for a device arena: one byte planted with a torch store, and
    the stores of a real kernel -- gmvae_noise_fill asked for one row more than its buffer holds writes 4 L bytes into the band
    behind it (memory this test owns: nothing faults) -- are both reported by name, side and distance."""
    rows, Lz, K = 33, 5, 3
    arena.reset()
    eps = arena.place("eps", 4 * rows * Lz, 4 * Lz, True, dtype=torch.float32)
    u = arena.place("u", 4 * rows * K, 4 * K, False, dtype=torch.float32)
    assert eps.is_cuda and eps.data_ptr() % 256 == 0 and u.data_ptr() % 256 == 0 and torch.isnan(eps).all()
    arena.snapshot()
    arena.mem[arena.buf("u").start - 1] = 0
    with pytest.raises(A.GuardHit) as e:
        arena.check()
    assert [(h["name"], h["side"], h["distance"], h["old"], h["new"]) for h in e.value.hits] == [("u", "front", 1, 255, 0)]
    arena.mem[arena.buf("u").start - 1] = 255
    arena.check()
    L.check(L.lib.gmvae_noise_fill(L.ptr(eps), None, rows + 1, Lz, K, 0, 1, 0, None, L.current_stream()), "noise")
    with pytest.raises(A.GuardHit) as e:
        arena.check()
    h, = e.value.hits
    assert (h["name"], h["side"], h["old"]) == ("eps", "behind", 255) and 1 <= h["distance"] <= h["farthest"] == 4 * Lz
    assert torch.isfinite(eps).all() and torch.isnan(u).all()


# ------------------------------------------------------------------------------------------------------ A: gmvae_step
@_of_kind("step")
def test_step_at_gate_corner_stays_inside_its_buffers(c, monkeypatch, H, L, arena):
    _set_env(monkeypatch, c)
    model, d, p, x, eps, u = _corner_inputs(c, c.B)
    assert L.step_schedule(H.dims_of(d, c.B), model) == c.sched
    with _Timed("A", arena):
        H.compare_step(model, d, p, x, eps, u, alloc=arena)
    ws = arena.buf("workspace")
    assert ws.nbytes == L.workspace_bytes(H.dims_of(d, c.B), model)              # exactly the size query, no slack
    assert arena.buf("grads").nbytes == 4 * (L.param_count(H.dims_of(d, c.B), model)[0] + L.TAIL)


PHILOX_CORNERS = ("mega-gmvae-B17", "fused-L8", "skinny-B129", "fused-L12")        # one per schedule word


@pytest.mark.parametrize("cid", PHILOX_CORNERS)
def test_step_with_kernel_noise_and_device_counter_stays_inside_its_buffers(cid, monkeypatch, H, L, arena):
    """eps = u = NULL and a step_dev: the two words of the counter are all the call may change of it, the counter goes up by
    one, x and params keep their bits, the tail is finite."""
    c = G.BY_ID[cid]
    _set_env(monkeypatch, c)
    model, d, p, x, _, _ = _corner_inputs(c, c.B)
    assert [G.BY_ID[i].sched for i in PHILOX_CORNERS] == ["mega", "fused", "skinny", "general"]
    flat = O.pack(model, d, p, np.float32)
    with _Timed("A", arena):
        arena.reset()
        cd = H.dims_of(d, c.B, arena)
        assert L.step_schedule(cd, model) == c.sched
        P, _ = L.param_count(cd, model)
        pitch = H.pitch_of(d)
        params = H.put(arena, "params", flat, torch.float32, pitch)
        xd = H.put(arena, "x", x, torch.uint8, d.D)
        grads = H.out(arena, "grads", (P + L.TAIL,), pitch)
        step_dev = arena.place("step_dev", 16, 16, True, dtype=torch.int64)
        step_dev[0], step_dev[1] = 41, 0
        ws = H.exact_workspace(arena, L.workspace_bytes(cd, model), pitch)
        H.run_checked(arena, "gmvae_step", lambda: L.lib.gmvae_step(
            C.byref(cd), model, L.ptr(xd), None, None, L.ptr(params), L.ptr(grads), L.ptr(ws), 7, 999, L.ptr(step_dev),
            L.current_stream()))
    assert int(step_dev[0]) == 42
    g = grads.cpu().numpy()
    assert np.isfinite(g[P:]).all() and g[P + 4] == c.B
    lay = L.param_layout(cd, model)
    for name, (r, cc), off in lay:
        assert np.isfinite(g[off:off + r * cc]).all(), name


# --------------------------------------------------------------------------------------------------- B: gmvae_forward
FORWARD_CORNERS = [c.id for c in G.CORNERS if c.kind == "evalf"] + ["mega-vae_gmp-B15", "fused-K64", "skinny-vae-L4", "skinny-B4097"]


@pytest.mark.parametrize("cid", FORWARD_CORNERS)
def test_forward_stays_inside_its_buffers(cid, monkeypatch, H, L, arena):
    c = G.BY_ID[cid]
    _set_env(monkeypatch, c)
    B = G.batch_on(c, _cus())
    model, d, p, x, eps, u = _corner_inputs(c, B)
    if c.kind == "step":
        assert L.step_schedule(H.dims_of(d, B), model) == c.sched
    flat = O.pack(model, d, p, np.float32)
    Cc = O.forward(model, d, O.unpack(model, d, flat.astype(np.float64)), x, eps, u)
    shapes = {"rows": (B, 4), "z": (B, d.L), "y": (B, d.K), "logits": (B, d.K)}
    for outputs in (H.FORWARD_OUTPUTS,) + tuple((k,) for k in H.FORWARD_OUTPUTS):
        with _Timed("B", arena):
            o = H.forward_in(arena, model, d, flat, x, eps, u, outputs=outputs)
        assert arena.buf("workspace").nbytes == L.workspace_bytes(H.dims_of(d, B), model)
        assert set(o) == {"tail"} | set(outputs)
        for k in outputs:
            assert o[k].shape == shapes[k] and arena.buf(k).nbytes == 4 * shapes[k][0] * shapes[k][1]
        assert o["tail"][0] / B == pytest.approx(Cc["loss"], rel=1e-5) and o["tail"][4] == B
        if "rows" in o:
            np.testing.assert_allclose(o["rows"][:, 0], Cc["logpx"], rtol=1e-5)
            np.testing.assert_allclose(o["rows"][:, 3], Cc["logw"], rtol=1e-5)
        if "z" in o:
            np.testing.assert_allclose(o["z"], Cc["z"], rtol=1e-4, atol=1e-5)
        if model == O.MODEL_GMVAE and "y" in o:
            np.testing.assert_allclose(o["y"], Cc["y"], rtol=1e-4, atol=1e-6)
        if model == O.MODEL_GMVAE and "logits" in o:
            np.testing.assert_allclose(o["logits"], Cc["logits"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------------ C: train graphs
HP = (1e-3, 0.9, 0.999, 1e-8)


def _train(alloc, L, H, model, d, B, xs, flat, graph_steps, seed=77):
    """len(xs) training steps through gmvae_train_graph_create on buffers of `alloc`: one launch of a len(xs)-step graph
    (graph_steps == len(xs): the batches back to back in one buffer, as the header lays them out) or len(xs) launches of a 1-step
    graph whose one batch buffer is refilled in between.  Writable: everything but x.  Returns params, m, v, tail_log as numpy."""
    n = len(xs)
    assert graph_steps in (1, n)
    alloc.reset()
    cd = H.dims_of(d, B, alloc)
    P, _ = L.param_count(cd, model)
    assert flat.shape == (P,)
    pitch = H.pitch_of(d)
    xd = alloc.place("x", graph_steps * B * d.D, d.D, False, dtype=torch.uint8)
    params = alloc.place("params", 4 * P, pitch, True, dtype=torch.float32)
    params.copy_(torch.from_numpy(flat))
    m = alloc.place("m", 4 * P, pitch, True, dtype=torch.float32).zero_()
    v = alloc.place("v", 4 * P, pitch, True, dtype=torch.float32).zero_()
    grads = H.out(alloc, "grads", (P + L.TAIL,), pitch)
    tail_log = H.out(alloc, "tail_log", (graph_steps, L.TAIL), 4 * L.TAIL)
    step_dev = alloc.place("step_dev", 16, 16, True, dtype=torch.int64).zero_()
    ws = H.exact_workspace(alloc, L.workspace_bytes(cd, model), pitch)
    assert alloc.view("workspace").numel() == L.workspace_bytes(cd, model)
    handle = C.c_void_p()
    tails = []
    try:
        for t in range(0, n, graph_steps):
            xd.copy_(torch.from_numpy(np.ascontiguousarray(xs[t:t + graph_steps])).reshape(-1))
            alloc.snapshot()
            if handle.value is None:
                torch.cuda.synchronize()
                L.check(L.lib.gmvae_train_graph_create(C.byref(cd), model, L.ptr(xd), graph_steps, L.ptr(params), L.ptr(m), L.ptr(v),
                                                       L.ptr(grads), L.ptr(ws), seed, L.ptr(step_dev), *HP, L.ptr(tail_log),
                                                       C.byref(handle)), "gmvae_train_graph_create")
            L.check(L.lib.gmvae_train_graph_launch(handle, L.current_stream()), "gmvae_train_graph_launch")
            alloc.check()
            tails.append(tail_log.cpu().numpy().copy())
    finally:
        torch.cuda.synchronize()
        if handle.value is not None:
            L.check(L.lib.gmvae_train_graph_destroy(handle), "gmvae_train_graph_destroy")
    assert int(step_dev[0]) == n
    return {"params": params.cpu().numpy(), "m": m.cpu().numpy(), "v": v.cpu().numpy(), "tail_log": np.concatenate(tails)}


def _train_inputs(model, d, B, n=3):
    xs = (np.random.default_rng(B).random((n, B, d.D)) < 0.87).astype(np.uint8)
    flat = O.pack(model, d, O.init_params(model, d, np.random.default_rng(B + 1)), np.float32)
    return xs, flat


@_of_kind("train")
def test_train_graph_at_gate_corner_stays_inside_its_buffers(c, monkeypatch, H, L, arena):
    _set_env(monkeypatch, c)
    model, d, B = O.MODEL_NAMES[c.model], c.d, G.batch_on(c, _cus())
    assert L.step_schedule(L.make_dims(B, d.D, d.L, d.K, d.hidden), model) == c.sched
    xs, flat = _train_inputs(model, d, B)
    with _Timed("C", arena):
        got = _train(arena, L, H, model, d, B, xs, flat, 3)
    want = _train(A.Plain("cuda"), L, H, model, d, B, xs, flat, 3)
    assert np.isfinite(got["tail_log"]).all() and (got["tail_log"][:, 4] == B).all()
    assert not np.array_equal(got["params"], flat)
    for k in ("params", "m", "v", "tail_log"):
        _same_bits(got[k], want[k], f"{c.id} {k}")


@pytest.mark.parametrize("D", [100, 97])
def test_train_graph_batches_at_unaligned_addresses(D, H, L, arena):
    """hidden = (), B = 9: the second and third batch of x [3][B][D] start 900 and 1800 bytes in (4-byte aligned) at D = 100,
    873 and 1746 bytes in (odd, even) at D = 97.  The 3-step graph against three launches of a 1-step graph that takes each
    batch from a 256-byte-aligned buffer, bit for bit, and both against plain allocations."""
    model, d, B = O.MODEL_GMVAE, O.Dims(D=D, L=5, K=7, hidden=()), 9
    xs, flat = _train_inputs(model, d, B)
    with _Timed("C", arena):
        three = _train(arena, L, H, model, d, B, xs, flat, 3)
    with _Timed("C", arena):
        ones = _train(arena, L, H, model, d, B, xs, flat, 1)
    plain = _train(A.Plain("cuda"), L, H, model, d, B, xs, flat, 3)
    assert np.isfinite(three["tail_log"]).all() and (three["tail_log"][:, 4] == B).all()
    for k in ("params", "m", "v", "tail_log"):
        _same_bits(three[k], ones[k], f"D={D} {k}: 3-step graph vs three 1-step graphs")
        _same_bits(three[k], plain[k], f"D={D} {k}: arena vs plain")


# -------------------------------------------------------------------------------- D: the objective and optimizer bits
SHAPE_D = dict(D=100, L=5, hidden=(24,))            # K = 7 (1 for the VAE), B = 9: nothing a multiple of 4 or 16, B D = 900
B_D = 9
EXTRAS = ("GRAD_DREG", "Y_STRAIGHT_THROUGH", "OPT_CLIP_NORM")
SIGMA_D = 0.5                                       # the caller-written "lik_sigma" cell of the fixed-scale Gaussian sets


def r256(n):
    return (n + 255) // 256 * 256


def _base_flags(L, y_inference, ge, want):
    f = {"gumbel": 0, "marginal": L.OBJ_MARGINAL_Y, "marginal_iw": L.OBJ_MARGINAL_Y_IW}[y_inference]
    f |= L.GRAD_DREG if ge == "dreg" else 0
    bit = {"semi_supervised": L.OBJ_LABELS, "weighted_objective": L.OBJ_WEIGHTS, "temperature_on_device": L.Y_TEMP_DEV,
           "pixel_mask": L.OBJ_PIXEL_MASK}
    for w in want:
        f |= bit[w]
    return f


def _extra_allowed(L, model, flags, extra):
    """include/gmvae_hip.h: GMVAE_GRAD_DREG covers the VAE family and the GMVAE with y summed out, not together with the
    weights or the mask; GMVAE_Y_STRAIGHT_THROUGH the Gumbel GMVAE, not together with the mask; GMVAE_OPT_CLIP_NORM everything."""
    marginal = flags & (L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW)
    if extra == "GRAD_DREG":
        return (model != "gmvae" or bool(marginal)) and not flags & (L.OBJ_WEIGHTS | L.OBJ_PIXEL_MASK)
    if extra == "Y_STRAIGHT_THROUGH":
        return model == "gmvae" and not marginal and not flags & L.OBJ_PIXEL_MASK
    return True


def _bit_sets(L, model, y_inference, ge, want):
    """[(flags, [S, ...])]: the construction's own set and the same with every subset of EXTRAS the header allows."""
    base = _base_flags(L, y_inference, ge, want)
    out = []
    for sub in range(1 << len(EXTRAS)):
        names = [e for i, e in enumerate(EXTRAS) if sub >> i & 1]
        f = base
        for e in names:
            f |= getattr(L, e)
        if f in [g for g, _ in out]:
            continue                                              # (the construction carries that bit already)
        cd = L.make_dims(B_D, 100, 5, 1 if model == "vae" else 7, (24,), sched_flags=f)
        if all(_extra_allowed(L, model, base, e) for e in names):
            assert L.workspace_bytes(cd, L.MODEL_IDS[model]) > 0
            out.append((f, [1] if f & (L.OBJ_MARGINAL_Y | L.OBJ_WEIGHTS) else [1, 3]))
        else:
            with pytest.raises(L.GmvaeError):                     # the library agrees with the rule above
                L.workspace_bytes(cd, L.MODEL_IDS[model])
    return out


def _fill_step_inputs(alloc, L, cd, model, ws, K, B, D, flags):
    """All 32 slots of every caller-written region get distinct valid values; the regions (each rounded up to 256 bytes, as the
    header sizes them) leave the workspace's writable set: the library only reads them."""
    wsb = alloc.view("workspace")
    n = wsb.numel()
    keep = []

    def region(name, nbytes, values):
        off = L.workspace_offset(cd, model, name)
        assert off % 256 == 0 and off + r256(nbytes) <= n
        raw = torch.from_numpy(np.ascontiguousarray(values)).reshape(-1).view(torch.uint8)
        assert raw.numel() <= nbytes
        wsb[off:off + raw.numel()].copy_(raw)
        keep.append((off, off + r256(nbytes)))

    S32 = L.LABEL_SLOTS
    s = np.arange(S32)
    if flags & L.OBJ_LABELS:
        B4 = (B + 3) // 4 * 4
        region("labels", 4 * S32 * B4, ((3 * s[:, None] + np.arange(B4)[None, :]) % (K + 1) - 1).astype(np.int32))
        region("sup_weight", 4, np.array([0.7], np.float32))
    if flags & L.OBJ_WEIGHTS:
        region("obj_weights", 16 * S32, np.stack([0.5 + 0.01 * s, 0.8 + 0.01 * s, 0.1 + 0.001 * s, 0 * s], 1).astype(np.float32))
    if flags & L.Y_TEMP_DEV:
        region("y_temperature", 4 * S32, (0.5 + 0.02 * s).astype(np.float32))
    if flags & L.OBJ_PIXEL_MASK:
        slot = r256(B * D)
        masks = np.zeros((S32, slot), np.uint8)
        masks[:, :B * D] = np.random.default_rng(5).random((S32, B * D)) < 0.8
        region("pixel_mask", S32 * slot, masks)
    if flags & L.OPT_CLIP_NORM:
        region("clip_norm", 4, np.array([2.5], np.float32))
    if flags & L.LIK_MASK == L.LIK_GAUSSIAN and not flags & L.LIK_SCALE_LEARNED:
        region("lik_sigma", 4, np.array([SIGMA_D], np.float32))
    keep.sort()
    free, at = [], 0
    for lo, hi in keep:
        assert lo >= at
        free.append((at, lo))
        at = hi
    free.append((at, n))
    alloc.set_writable("workspace", free)


def _flagged_call(alloc, L, H, entry, name, d, B, flags, flat, x, eps, u):
    model = L.MODEL_IDS[name]

    def prepare(cd, ws):
        _fill_step_inputs(alloc, L, cd, model, ws, d.K, B, d.D, flags)
    if entry == "forward":
        return H.forward_in(alloc, model, d, flat, x, eps, u, flags=flags, prepare=prepare)
    alloc.reset()
    cd = H.dims_of(d, B, alloc)
    cd.sched_flags = flags
    P, _ = L.param_count(cd, model)
    pitch = H.pitch_of(d)
    params = H.put(alloc, "params", flat, torch.float32, pitch)
    xd = H.put_x(alloc, x, d.D)
    ed = H.put(alloc, "eps", eps, torch.float32, 4 * d.L)
    ud = None if u is None else H.put(alloc, "u", u, torch.float32, 4 * d.K)
    grads = H.out(alloc, "grads", (P + L.TAIL,), pitch)
    ws = H.exact_workspace(alloc, L.workspace_bytes(cd, model), pitch)
    prepare(cd, ws)
    H.run_checked(alloc, "gmvae_step", lambda: L.lib.gmvae_step(
        C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 0, None,
        L.current_stream()))
    g = grads.cpu().numpy()
    if flags & L.OPT_CLIP_NORM:
        # "the padding words of the gradient buffer ... are zero after every step": every alignment-padding word, from 0xFF, is +0.0
        real = np.zeros(P, bool)
        for _, (r, c), off in L.param_layout(cd, model):
            real[off:off + r * c] = True
        pad = g[:P].view(np.uint32)[~real]
        assert pad.size and (pad == 0).all(), (name, hex(flags), pad)
    return {"grads": g}


@pytest.mark.parametrize("args,want", CONSTRUCTIONS, ids=["-".join(map(str, a[:4])) + "-" + ("+".join(w) or "none") for a, w in CONSTRUCTIONS])
def test_objective_and_optimizer_bits_stay_inside_their_buffers(args, want, H, L, arena):
    name, y_inference, _, ge = args[:4]
    K = 1 if name == "vae" else 7
    sets = _bit_sets(L, name, y_inference, ge, want)
    assert sets
    rng = np.random.default_rng(len(want) + K)
    for flags, samples in sets:
        for S in samples:
            d = O.Dims(K=K, S=S, **SHAPE_D)
            model = O.MODEL_NAMES[name]
            flat = O.pack(model, d, O.init_params(model, d, rng), np.float32)
            x = (rng.random((B_D, d.D)) < 0.6).astype(np.uint8)
            marginal = flags & (L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW)
            eps = rng.standard_normal((B_D * S * (K if marginal else 1), d.L)).astype(np.float32)
            u = rng.uniform(0.05, 0.95, (B_D * S, K)).astype(np.float32) if name == "gmvae" and not marginal else None
            for entry in ("step", "forward"):
                with _Timed("D", arena):
                    got = _flagged_call(arena, L, H, entry, name, d, B_D, flags, flat, x, eps, u)
                cd = H.dims_of(d, B_D)
                cd.sched_flags = flags
                assert arena.buf("workspace").nbytes == L.workspace_bytes(cd, model)
                ref = _flagged_call(A.Plain("cuda"), L, H, entry, name, d, B_D, flags, flat, x, eps, u)
                tail = got["grads"][-L.TAIL:] if entry == "step" else got["tail"]
                assert np.isfinite(tail).all() and tail[4] == B_D, (entry, hex(flags), S, tail)
                for k in got:
                    _same_bits(got[k], ref[k], f"{name} flags {flags:#x} S={S} {entry} {k}")


# the likelihood bits (GMVAE_LIK_*, GMVAE_X_F32, GMVAE_LIK_SCALE_LEARNED): under GMVAE_X_F32 the caller's x is 4 B D bytes of
# floats, read 16 bytes at a time as a GEMM operand (the first layers and their weight gradients, ragged tiles included) and as
# the likelihood epilogue's target; "lik_sigma" is a caller-written workspace cell
LIK_SETS = {"grey": ("LIK_GREY_BERNOULLI",), "cb": ("LIK_CONT_BERNOULLI",), "gauss": ("LIK_GAUSSIAN",),
            "gauss+f32": ("LIK_GAUSSIAN", "X_F32"), "gauss+lsig": ("LIK_GAUSSIAN", "LIK_SCALE_LEARNED"),
            "gauss+f32+lsig": ("LIK_GAUSSIAN", "X_F32", "LIK_SCALE_LEARNED")}


@pytest.mark.parametrize("name", G.MODELS)
@pytest.mark.parametrize("lset", list(LIK_SETS))
def test_likelihood_bits_stay_inside_their_buffers(lset, name, monkeypatch, H, L, arena):
    """Group D under every likelihood flag set, with and without GMVAE_OPT_CLIP_NORM: B = 9, S in {1, 3}, D = 100 and D = 99
    (float rows that are not 16-byte aligned), gmvae_step -- once more under GMVAE_FORCE_CFG=2: 128-row tiles over 9 rows read x
    as an operand -- and gmvae_forward; x at exactly its bytes and read-only, "lik_sigma" read-only; the guards untouched, the
    tail finite, every output the bits of the same call in plain allocations."""
    import lik_ref
    import realx_ref
    base = 0
    for f in LIK_SETS[lset]:
        base |= getattr(L, f)
    f32, learned = bool(base & L.X_F32), bool(base & L.LIK_SCALE_LEARNED)
    K = 1 if name == "vae" else 7
    model = O.MODEL_NAMES[name]
    for illegal in ("GRAD_DREG", "Y_STRAIGHT_THROUGH"):                 # the library agrees that these do not combine
        cd = L.make_dims(B_D, 100, 5, K, (24,), sched_flags=base | getattr(L, illegal))
        with pytest.raises(L.GmvaeError):
            L.workspace_bytes(cd, L.MODEL_IDS[name])
    rng = np.random.default_rng(len(lset) + K)
    for flags in (base, base | L.OPT_CLIP_NORM):
        for D in (100, 99):
            xf, rho = realx_ref.real_batch(B_D, D)
            x = xf if f32 else lik_ref.grey_batch(B_D, D)
            for S in (1, 3):
                d = O.Dims(D=D, L=5, hidden=(24,), K=K, S=S)
                flat = O.pack(model, d, O.init_params(model, d, rng), np.float32)
                if learned:
                    flat = np.concatenate([flat, rho, np.zeros(-D % 4, np.float32)])
                eps = rng.standard_normal((B_D * S, d.L)).astype(np.float32)
                u = rng.uniform(0.05, 0.95, (B_D * S, K)).astype(np.float32) if name == "gmvae" else None
                for entry, cfg in (("step", None), ("step", "2"), ("forward", None)):
                    for k in G.SWITCHES + ("GMVAE_FORCE_CFG", "GMVAE_NO_BIG"):
                        monkeypatch.delenv(k, raising=False)
                    if cfg:
                        monkeypatch.setenv("GMVAE_FORCE_CFG", cfg)
                    what = f"{name} {lset} flags {flags:#x} D={D} S={S} {entry} cfg {cfg}"
                    with _Timed("D", arena):
                        got = _flagged_call(arena, L, H, entry, name, d, B_D, flags, flat, x, eps, u)
                    cd = H.dims_of(d, B_D)
                    cd.sched_flags = flags
                    assert arena.buf("workspace").nbytes == L.workspace_bytes(cd, model)
                    assert arena.buf("x").nbytes == (4 if f32 else 1) * B_D * D and arena.buf("x").writable == []
                    assert arena.buf("params").nbytes == 4 * L.param_count(cd, model)[0]
                    ref = _flagged_call(A.Plain("cuda"), L, H, entry, name, d, B_D, flags, flat, x, eps, u)
                    tail = got["grads"][-L.TAIL:] if entry == "step" else got["tail"]
                    assert np.isfinite(tail).all() and tail[4] == B_D and tail[6] == B_D * D, (what, tail)
                    if entry == "step":
                        assert np.isfinite(got["grads"]).all(), what
                    for k in got:
                        _same_bits(got[k], ref[k], f"{what} {k}")


# ------------------------------------------------------------- E: the chunked evaluators and the small entry points
CHUNKED = [("iw_bound", "gmvae"), ("iw_bound_enum_y", "gmvae"), ("posterior_y", "gmvae"), ("posterior_component", "vae_gmp")]


@pytest.mark.parametrize("kind,name", CHUNKED, ids=[k for k, _ in CHUNKED])
def test_chunked_evaluators_stay_inside_their_buffers(kind, name, H, L, arena):
    """n = 7 samples in chunks of 3 (the last chunk partial), every optional output omitted in turn."""
    model, d, B = O.MODEL_NAMES[name], O.Dims(K=7, **SHAPE_D), B_D
    rng = np.random.default_rng(11)
    flat = O.pack(model, d, O.init_params(model, d, rng), np.float32)
    x = (rng.random((B, d.D)) < 0.6).astype(np.uint8)
    for omit in [()] + [(k,) for k in H.CHUNKED_OUTPUTS[kind]]:
        with _Timed("E", arena):
            got = H.chunked_call(kind, model, d, flat, x, 7, 3, seed=3, step=2, omit=omit, alloc=arena)
        cd = H.dims_of(dataclasses.replace(d, S=3), B)
        assert arena.buf("workspace").nbytes == getattr(L, f"{kind}_workspace_bytes")(cd, model)
        ref = H.chunked_call(kind, model, d, flat, x, 7, 3, seed=3, step=2, omit=omit, alloc=A.Plain("cuda"))
        assert set(got) == set(H.CHUNKED_OUTPUTS[kind]) - set(omit) | {"tail"}
        for k in got:
            assert np.isfinite(got[k]).all(), (kind, omit, k)
            _same_bits(got[k], ref[k], f"{kind} without {omit}: {k}")


def _put(arena, name, a, dtype, pitch, writable=False):
    """hip_util.put, writable where the call under test updates the buffer in place."""
    import hip_util
    t = hip_util.put(arena, name, a, dtype, pitch)
    arena.set_writable(name, writable)
    return t


@pytest.mark.parametrize("P", [1, 5, 1023, 1028])
def test_adam_tf_step_stays_inside_its_buffers(P, L, arena):
    """params, m, v and grads of exactly P floats (tests/test_hip_parity.py pads them by one)."""
    rng = np.random.default_rng(P)
    th, g = rng.normal(size=P).astype(np.float32), rng.normal(size=P).astype(np.float32)
    m, v = (0.1 * rng.normal(size=P)).astype(np.float32), (0.01 * rng.random(P)).astype(np.float32)
    with _Timed("E", arena):
        arena.reset()
        td, md, vd = (_put(arena, n, a, torch.float32, 4, True) for n, a in (("params", th), ("m", m), ("v", v)))
        gd = _put(arena, "grads", g * 8.0, torch.float32, 4)
        arena.snapshot()
        L.check(L.lib.adam_tf_step(L.ptr(td), L.ptr(md), L.ptr(vd), L.ptr(gd), P, 1e-3, 0.9, 0.999, 1e-8, 2, None, 1.0 / 8.0, None,
                                   None, L.current_stream()), "adam")
        arena.check()
    th1, m1, v1 = O.adam_tf_step(th, m, v, g, 2, dtype=np.float32)
    np.testing.assert_allclose(td.cpu().numpy(), th1, rtol=2e-6, atol=2e-7)
    np.testing.assert_allclose(vd.cpu().numpy(), v1, rtol=2e-6, atol=1e-30)
    np.testing.assert_allclose(md.cpu().numpy(), m1, rtol=2e-6, atol=5e-8)


@pytest.mark.parametrize("P", [4, 1024, 1028])
def test_grad_clip_stays_inside_its_buffers(P, L, arena):
    import clip_ref
    rng = np.random.default_rng(P)
    b = np.zeros(P + clip_ref.TAIL, np.float32)
    b[:P] = rng.standard_normal(P)
    b[P], b[P + 4] = -12.5, 16.0
    for ratio in (0.5, 10.0):
        Cv = float(np.float32(ratio * clip_ref.record(b, math.inf)[0]))
        assert not clip_ref.flag_band(b, Cv)
        with _Timed("E", arena):
            arena.reset()
            gd = _put(arena, "grads", b, torch.float32, 4)
            cn = _put(arena, "clip_norm", np.array([Cv], np.float32), torch.float32, 4)
            rec = arena.place("rec", 16, 16, True, dtype=torch.float32)
            scratch = arena.place("scratch", L.grad_clip_scratch_bytes(P), 8, True, dtype=torch.float64)
            arena.snapshot()
            L.check(L.lib.gmvae_grad_clip(L.ptr(gd), P, L.ptr(cn), L.ptr(rec), L.ptr(scratch), L.current_stream()), "gmvae_grad_clip")
            arena.check()
        r = rec.cpu().numpy()
        clip_ref.check_record(r, b, Cv)
        assert bool(r[2]) == (ratio < 1)


@pytest.mark.parametrize("which", ["both", "eps", "u"])
def test_noise_fill_stays_inside_its_buffers(which, L, arena):
    rows, Lz, K, row_base = 33, 5, 3, 7
    with _Timed("E", arena):
        arena.reset()
        eps = arena.place("eps", 4 * rows * Lz, 4 * Lz, True, dtype=torch.float32) if which != "u" else None
        u = arena.place("u", 4 * rows * K, 4 * K, True, dtype=torch.float32) if which != "eps" else None
        arena.snapshot()
        L.check(L.lib.gmvae_noise_fill(L.ptr(eps), L.ptr(u), rows, Lz, K, row_base, 0xDEADBEEF12345, 9, None, L.current_stream()),
                "noise")
        arena.check()
    e_ref, u_ref = O.noise(rows, Lz, K, row_base, 0xDEADBEEF12345, 9)
    if u is not None:
        assert np.array_equal(u.cpu().numpy().reshape(rows, K), u_ref)
    if eps is not None:
        np.testing.assert_allclose(eps.cpu().numpy().reshape(rows, Lz), e_ref, rtol=0, atol=2e-5)


@pytest.mark.parametrize("D", [4, 100])
@pytest.mark.parametrize("by_idx", [True, False], ids=["idx", "row0"])
def test_binarize_stays_inside_its_buffers(D, by_idx, L, arena):
    """Source rows 0 and n_rows - 1 through idx; idx = NULL with row0 + B == n_rows: the last row read is the last one there."""
    B, n_rows, seed, step, out_row0 = 3, 10, 0xABCDEF, 4, 6
    pix = np.random.default_rng(D).integers(0, 256, (n_rows, D), dtype=np.uint8)
    rows = np.array([0, n_rows - 1, 4], np.int32) if by_idx else np.arange(n_rows - B, n_rows, dtype=np.int32)
    with _Timed("E", arena):
        arena.reset()
        pd = _put(arena, "pixels", pix, torch.uint8, D)
        idx = _put(arena, "idx", rows, torch.int32, 4 * B) if by_idx else None
        xo = arena.place("x_out", B * D, D, True, dtype=torch.uint8)
        arena.snapshot()
        L.check(L.lib.gmvae_binarize(L.ptr(pd), n_rows, L.ptr(idx), 0 if by_idx else n_rows - B, B, D, seed, step, None, L.ptr(xo),
                                     out_row0, L.current_stream()), "gmvae_binarize")
        arena.check()
    assert np.array_equal(xo.cpu().numpy().reshape(B, D), O.binarize(pix, rows, seed, step, out_row0))


def test_cluster_acc_stays_inside_its_buffers(L, arena):
    """scratch of exactly K * n_labels + B int32, 0xFF at first: the callee zeroes the histogram."""
    B, K, n_labels = 33, 7, 10
    rng = np.random.default_rng(0)
    logits, labels = rng.normal(size=(B, K)).astype(np.float32), rng.integers(0, n_labels, B)
    with _Timed("E", arena):
        arena.reset()
        ld = _put(arena, "logits", logits, torch.float32, 4 * K)
        lab = _put(arena, "labels", labels, torch.int64, 8)
        scratch = arena.place("scratch", 4 * (K * n_labels + B), 4 * n_labels, True, dtype=torch.int32)
        acc = arena.place("acc", 4, 4, True, dtype=torch.float32)
        arena.snapshot()
        L.check(L.lib.gmvae_cluster_acc(L.ptr(ld), L.ptr(lab), B, K, n_labels, L.ptr(scratch), L.ptr(acc), L.current_stream()),
                "cluster_acc")
        arena.check()
    want = np.zeros((K, n_labels), np.int32)
    np.add.at(want, (logits.argmax(1), labels), 1)
    assert np.array_equal(scratch[:K * n_labels].cpu().numpy().reshape(K, n_labels), want)
    assert np.array_equal(scratch[K * n_labels:].cpu().numpy(), logits.argmax(1))
    assert acc.item() == pytest.approx(O.cluster_acc(logits, labels, K), abs=1e-6)


MLP_NETS = {"gmvae": ("ENCODER_Y", "PRIOR_GMM", "ENCODER_GMM", "DECODER"), "vae": ("ENCODER", "DECODER"), "vae_gmp": ("ENCODER", "DECODER")}


@pytest.mark.parametrize("name,net", [(m, n) for m, ns in MLP_NETS.items() for n in ns], ids=lambda v: str(v).lower())
def test_mlp_forward_stays_inside_its_buffers(name, net, H, L, arena):
    """Every sub-network of every model on 9 rows at group D's shape, against snt.nets.MLP restated in fp64 (oracle._mlp_fwd)."""
    from oracle import gmvae_oracle as OO
    rows, model = 9, O.MODEL_NAMES[name]
    d = O.Dims(K=1 if name == "vae" else 7, gen_bias_init=-0.3, **SHAPE_D)
    rng = np.random.default_rng(rows + len(net))
    p = O.init_params(model, d, rng)
    for k in p:
        if k.endswith("/b"):
            p[k] = rng.normal(0, 0.05, p[k].shape)
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    x = (rng.random((rows, d.D)) < 0.6).astype(np.uint8)
    y = rng.dirichlet(np.ones(d.K), rows).astype(np.float32)
    z = rng.standard_normal((rows, d.L)).astype(np.float32)
    n_layers = len(d.hidden) + 1
    inp, in2, out_dim, ref = {
        "ENCODER_Y": lambda: (x, None, d.K, OO._mlp_fwd(p32, "encoder_y", n_layers, x.astype(np.float64))[0]),
        "PRIOR_GMM": lambda: (y, None, 2 * d.L, OO._mlp_fwd(p32, "prior_gmm", 1, y.astype(np.float64))[0]),
        "ENCODER_GMM": lambda: (x, y, 2 * d.L, OO._mlp_fwd(p32, "encoder_gmm", n_layers, np.concatenate([x, y], 1).astype(np.float64))[0]),
        "DECODER": lambda: (z, None, d.D, OO._mlp_fwd(p32, "decoder", n_layers, z.astype(np.float64))[0] + d.gen_bias_init),
        "ENCODER": lambda: (x, None, 2 * d.L, OO._mlp_fwd(p32, "encoder", n_layers, x.astype(np.float64))[0]),
    }[net]()
    u8 = inp.dtype == np.uint8
    with _Timed("E", arena):
        arena.reset()
        cd = H.dims_of(d, rows, arena)
        pitch = H.pitch_of(d)
        params = H.put(arena, "params", flat, torch.float32, pitch)
        ind = H.put(arena, "in", inp, torch.uint8 if u8 else torch.float32, inp.shape[1] * (1 if u8 else 4))
        in2d = None if in2 is None else H.put(arena, "in2", in2, torch.float32, 4 * d.K)
        od = H.out(arena, "out", (rows, out_dim), 4 * out_dim)
        ws = H.exact_workspace(arena, L.workspace_bytes(cd, model), pitch)
        H.run_checked(arena, "gmvae_mlp_forward", lambda: L.lib.gmvae_mlp_forward(
            C.byref(cd), model, getattr(L, f"NET_{net}"), L.ptr(ind), int(u8), L.ptr(in2d), rows, L.ptr(params), L.ptr(od), L.ptr(ws),
            L.current_stream()))
    np.testing.assert_allclose(od.cpu().numpy(), ref, rtol=1e-4, atol=1e-5)


def _gemm(arena, L, A_, u8, W, bias, c_shape, M, N, K, trans, relu, cfg, ns):
    """One gmvae_gemm_test call on exact-size operands in the arena; C as numpy."""
    arena.reset()
    Ad = _put(arena, "A", A_, torch.uint8 if u8 else torch.float32, A_.shape[1] * (1 if u8 else 4))
    Wd = _put(arena, "W", W, torch.float32, 4 * W.shape[1])
    bd = None
    if bias is not None:
        bd = Wd if bias is W else _put(arena, "bias", bias, torch.float32, 4 * bias.shape[-1])
    Cd = arena.place("C", 4 * int(np.prod(c_shape)), 4 * c_shape[-1], True, dtype=torch.float32)
    arena.snapshot()
    L.check(L.lib.gmvae_gemm_test(L.ptr(Ad), int(u8), L.ptr(Wd), L.ptr(bd), L.ptr(Cd), M, N, K, trans, relu, cfg, ns,
                                  L.current_stream()), "gemm_test")
    arena.check()
    return Cd.cpu().numpy().reshape(c_shape).astype(np.float64)


GEMMS = [("nn", 7, 3, 5, False, 1), ("nn", 130, 131, 33, False, 1), ("nn", 33, 10, 784, True, 1), ("nt", 31, 784, 64, False, 1),
         ("tn", 65, 33, 70, False, 16)]


@pytest.mark.parametrize("cfg", [0, 1, 2])
@pytest.mark.parametrize("form,M,N,K,u8,ns", GEMMS, ids=[f"{g[0]}-{g[1]}x{g[2]}x{g[3]}" for g in GEMMS])
def test_gemm_stays_inside_its_buffers(cfg, form, M, N, K, u8, ns, L, arena):
    """The grouped fp32-MFMA kernel in every tile configuration on ragged shapes, C of exactly M N floats (TN: ns slabs of
    (M + 1) N), against fp64 at tests/test_hip_parity.py's tolerances."""
    rng = np.random.default_rng(M * 1000 + N)
    with _Timed("E", arena):
        if form == "nn":
            A_ = (rng.random((M, K)) < 0.5).astype(np.uint8) if u8 else rng.normal(size=(M, K)).astype(np.float32)
            W, b = rng.normal(size=(K, N)).astype(np.float32), rng.normal(size=N).astype(np.float32)
            got = _gemm(arena, L, A_, u8, W, b, (M, N), M, N, K, 0, 1, cfg, 1)
            ref, atol = np.maximum(A_.astype(np.float64) @ W.astype(np.float64) + b, 0), 2e-5 * math.sqrt(K)
        elif form == "nt":
            A_, W = rng.normal(size=(M, K)).astype(np.float32), rng.normal(size=(N, K)).astype(np.float32)
            got = _gemm(arena, L, A_, False, W, None, (M, N), M, N, K, 1, 0, cfg, 1)
            ref, atol = A_.astype(np.float64) @ W.astype(np.float64).T, 2e-5 * math.sqrt(K)
        else:
            A_, W = rng.normal(size=(K, M)).astype(np.float32), rng.normal(size=(K, N)).astype(np.float32)
            got = _gemm(arena, L, A_, False, W, W, (ns, M + 1, N), M, N, K, 2, 0, cfg, ns).sum(axis=0)
            ref = np.concatenate([A_.astype(np.float64).T @ W, W.astype(np.float64).sum(0, keepdims=True)], 0)
            atol = 3e-5 * math.sqrt(K)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=atol)


@pytest.mark.parametrize("form,M,N,K", [("nn", 37, 128, 64), ("nt_k8", 5, 64, 512)])
def test_rows_weight_stationary_stays_inside_its_buffers(form, M, N, K, L, arena):
    """csrc/rowsws.hpp (`cfg` 8) with more waves than rows: C of exactly M rows (tests/test_hip_parity.py appends three)."""
    rng = np.random.default_rng(M * 7 + N + K)
    A_ = rng.normal(size=(M, K)).astype(np.float32)
    A_[rng.random((M, K)) < 0.1] = 0.0
    with _Timed("E", arena):
        if form == "nn":
            W, side = rng.normal(size=(K, N)).astype(np.float32), rng.normal(size=N).astype(np.float32)
            got = _gemm(arena, L, A_, False, W, side, (M, N), M, N, K, 0, 1, 8, 1)
            ref = np.maximum(A_.astype(np.float64) @ W.astype(np.float64) + side, 0)
        else:
            W = rng.normal(size=(N, K)).astype(np.float32)
            got = _gemm(arena, L, A_, False, W, None, (M, N), M, N, K, 1, 0, 8, 1)
            ref = A_.astype(np.float64) @ W.astype(np.float64).T
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-6 * math.sqrt(K))


def test_memory_contract_report(arena):
    """Not a gate: what the groups above measured in this process (file order, run with -s) -- the source of the table in
    profiles/memory_contract_notes.md."""
    print()
    for group, (cases, used, secs) in sorted(STATS.items()):
        print(f"[memory contract] group {group}: {cases} guarded calls, largest arena {used} bytes, {secs:.3f} s")
    print(f"[memory contract] arena peak {arena.peak} of {arena.capacity} bytes")
