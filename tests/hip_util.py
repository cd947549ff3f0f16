"""Helpers for the -m gpu parity tests: call the C ABI with torch device buffers.

hip_step, hip_forward, forward_call, chunked_call and compare_step take an optional alloc= (tests/arena.py): every device buffer
of the call, dims_of's gen_bias_vec included, then lies in that arena at its exact size -- the workspace at exactly the bytes its
size query answers, zeroed; every output 0xFF -- and the arena's check() runs before the results come back."""
import ctypes as C
import dataclasses

import numpy as np
import torch

import oracle as O
from gmvae_amd import _lib as L


def dims_of(d: O.Dims, B: int, alloc=None):
    gb = np.asarray(d.gen_bias_init, np.float32)
    vec = torch.from_numpy(gb.copy()).cuda() if gb.ndim else None        # vector bias_init (ABI v3)
    if alloc is not None and gb.ndim:
        vec = put(alloc, "gen_bias_vec", gb, torch.float32, 4 * d.D)
    cd = L.make_dims(B, d.D, d.L, d.K, d.hidden, S=d.S, sigma_min=d.sigma_min, raw_sigma_bias=d.raw_sigma_bias,
                     temperature=d.temperature, gen_bias_init=0.0 if gb.ndim else float(gb), gen_bias_vec=vec,
                     hidden_act=getattr(d, "act", "relu"))
    cd._keep_vec = vec                                                    # the struct holds a raw device pointer
    return cd


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def workspace(cd, model):
    return torch.zeros(L.workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")


# ---- alloc=: the same calls with every device buffer inside a guarded arena (tests/arena.py; tests/test_memory_contract.py) ----
def pitch_of(d):
    """The longest row, in bytes, of any fp32 matrix a call of these dims stores: the arena's guard bands follow it."""
    return 4 * max(d.D, 2 * d.L, d.K, *d.hidden)


def put(alloc, name, a, dtype, pitch):
    """A read-only input placed in `alloc` and filled from the host array `a`."""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).reshape(-1)
    v = alloc.place(name, t.numel() * t.element_size(), pitch, False, dtype=dtype)
    v.copy_(t)
    return v


def put_x(alloc, x, D):
    """The batch placed in `alloc` at exactly its bytes, read-only: uint8 [B, D] as B D bytes, float32 [B, D] (GMVAE_X_F32) as
    4 B D bytes."""
    f32 = np.asarray(x).dtype == np.float32
    return put(alloc, "x", x, torch.float32 if f32 else torch.uint8, 4 * D if f32 else D)


def out(alloc, name, shape, pitch):
    """A writable fp32 output placed in `alloc`: every byte 0xFF (a NaN) until the call writes it."""
    return alloc.place(name, 4 * int(np.prod(shape)), pitch, True, dtype=torch.float32).view(*shape)


def exact_workspace(alloc, nbytes, pitch, name="workspace"):
    """The workspace at exactly the bytes its size query answered, zeroed, writable, as a float32 view."""
    assert nbytes % 4 == 0
    ws = alloc.place(name, nbytes, pitch, True, dtype=torch.float32)
    ws.zero_()
    return ws


def run_checked(alloc, what, call):
    """snapshot, the call, check: GuardHit if a byte changed outside the writable set."""
    alloc.snapshot()
    L.check(call(), what)
    alloc.check()


def _hip_step_in(alloc, model, d, flat, x, eps, u, seed, step, want_masks):
    alloc.reset()
    B = x.shape[0]
    cd = dims_of(d, B, alloc)
    P, _ = L.param_count(cd, model)
    pitch = pitch_of(d)
    params = put(alloc, "params", flat, torch.float32, pitch)
    xd = put(alloc, "x", x, torch.uint8, d.D)
    ed = None if eps is None else put(alloc, "eps", eps, torch.float32, 4 * d.L)
    ud = None if u is None else put(alloc, "u", u, torch.float32, 4 * d.K)
    grads = out(alloc, "grads", (P + L.TAIL,), pitch)                     # writable: grads[0, P_padded + 8)
    ws = exact_workspace(alloc, L.workspace_bytes(cd, model), pitch)
    run_checked(alloc, "gmvae_step", lambda: L.lib.gmvae_step(
        C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws), seed, step, None,
        L.current_stream()))
    g = grads.cpu().numpy().astype(np.float64)
    if want_masks:
        return g[:P], g[P:], device_masks(ws, cd, model, d, B)
    return g[:P], g[P:]


FORWARD_OUTPUTS = ("rows", "z", "y", "logits")


def forward_in(alloc, model, d, flat, x, eps, u, row0=0, flags=0, seed=0, step=0, outputs=FORWARD_OUTPUTS, prepare=None):
    """gmvae_forward at d.S samples with every buffer in `alloc` (x uint8, or float32 under GMVAE_X_F32): dict of tail [8] and the
    optional outputs named in `outputs`
    (rows [R, 4], z [R, L], y [R, K], logits [B, K]; the others are passed as NULL) as numpy.  prepare(cd, ws): fills the
    caller-written workspace regions and narrows the writable set before the call."""
    alloc.reset()
    B = x.shape[0]
    cd = dims_of(d, B, alloc)
    cd.row0, cd.sched_flags = row0, flags
    R = B * d.S * (d.K if flags & (L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW) else 1)
    pitch = pitch_of(d)
    params = put(alloc, "params", flat, torch.float32, pitch)
    xd = put_x(alloc, x, d.D)
    ed = None if eps is None else put(alloc, "eps", eps, torch.float32, 4 * d.L)
    ud = None if u is None else put(alloc, "u", u, torch.float32, 4 * d.K)
    shapes = {"rows": (R, 4), "z": (R, d.L), "y": (R, d.K), "logits": (B, d.K)}
    o = {"tail": out(alloc, "tail", (L.TAIL,), 4 * L.TAIL)}
    for k in FORWARD_OUTPUTS:
        o[k] = out(alloc, k, shapes[k], 4 * shapes[k][1]) if k in outputs else None
    ws = exact_workspace(alloc, L.workspace_bytes(cd, model), pitch)
    if prepare is not None:
        prepare(cd, ws)
    run_checked(alloc, "gmvae_forward", lambda: L.lib.gmvae_forward(
        C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(o["tail"]), L.ptr(o["rows"]), L.ptr(o["z"]),
        L.ptr(o["y"]), L.ptr(o["logits"]), L.ptr(ws), seed, step, L.current_stream()))
    return {k: t.cpu().numpy() for k, t in o.items() if t is not None}


def chunked_in(alloc, kind, model, d, flat, x, n, chunk, row0=0, flags=0, seed=0, step=0, omit=()):
    """chunked_call with every buffer in `alloc`, the workspace at exactly gmvae_<kind>_workspace_bytes."""
    alloc.reset()
    B = x.shape[0]
    cd = dims_of(dataclasses.replace(d, S=chunk), B, alloc)
    cd.row0, cd.sched_flags = row0, flags
    pitch = pitch_of(d)
    shape = {"bound": (B,), "mean_logw": (B,), "log_joint": (B, d.K), "log_post": (B, d.K), "stats": (B, 4)}
    o = {k: None if k in omit else out(alloc, k, shape[k], 4 * shape[k][-1]) for k in CHUNKED_OUTPUTS[kind]}
    o["tail"] = out(alloc, "tail", (L.TAIL,), 4 * L.TAIL)
    params = put(alloc, "params", flat, torch.float32, pitch)
    xd = put(alloc, "x", x, torch.uint8, d.D)
    ws = exact_workspace(alloc, getattr(L, f"{kind}_workspace_bytes")(cd, model), pitch)
    run_checked(alloc, f"gmvae_{kind}", lambda: getattr(L.lib, f"gmvae_{kind}")(
        C.byref(cd), model, L.ptr(xd), L.ptr(params), n, *(L.ptr(t) for t in o.values()), L.ptr(ws), seed, step,
        L.current_stream()))
    return {k: t.cpu().numpy() for k, t in o.items() if t is not None}


NETS = {O.MODEL_GMVAE: (("encoder_y", "he", False), ("encoder_gmm", "hg", True), ("decoder", "hd", True)),
        O.MODEL_VAE: (("encoder", "he", False), ("decoder", "hd", True)),
        O.MODEL_VAE_GMP: (("encoder", "he", False), ("decoder", "hd", True))}
PRE_TOL = 1e-5         # a ReLU may take the other side than in fp64 only where |pre-activation| <= PRE_TOL * sum_k |a_k| |w_kj|
FLIPS = []             # (what, net, |pre| / sum |a||w|) of every unit where a compared step's ReLU mask differed from fp64's


def device_masks(ws, cd, model, d, B):
    """The ReLU masks of the step that last ran in workspace `ws` (a float32 device tensor): (kept activation > 0) of every
    hidden layer (gmvae_workspace_offset "he<i>" / "hg<i>" / "hd<i>"; rows = B for the encoder of x, B*S otherwise)."""
    out = {}
    for net, tag, per_sample in NETS[model]:
        ms = [None]
        for i, h in enumerate(d.hidden, start=1):
            off = C.c_uint64()
            L.check(L.lib.gmvae_workspace_offset(C.byref(cd), model, f"{tag}{i}".encode(), C.byref(off)), f"offset {tag}{i}")
            rows = B * d.S if per_sample else B
            ms.append(ws[off.value // 4: off.value // 4 + rows * h].view(rows, h).cpu().numpy() > 0)
        out[net] = ms
    return out


def check_masks(masks, pres, what):
    """Every unit where the device's mask differs from the fp64 one must be numerically zero in fp64 (PRE_TOL); returns the
    number of such units."""
    n = 0
    for net, ms in masks.items():
        for i in range(1, len(ms)):
            pre, mag = pres[net][i - 1]
            diff = ms[i] != (pre > 0)
            if diff.any():
                ratio = np.abs(pre[diff]) / np.maximum(mag[diff], 1e-30)
                FLIPS.extend((what, net, float(r)) for r in ratio)
                n += int(diff.sum())
                assert ratio.max() <= PRE_TOL, (f"{what} {net} layer {i}: the device's ReLU mask differs from fp64's at a "
                                                f"pre-activation that is NOT numerically zero (|pre| / sum|a||w| = {ratio.max():.2e})")
    return n


INPUT_DTYPES = {"labels": np.int32, "pixel_mask": np.uint8}        # of the per-step inputs' regions; every other one is fp32


def write_inputs(ws, cd, model, inputs):
    """Slot 0 of the caller-written workspace regions: inputs = {region name (gmvae_workspace_offset's: labels, sup_weight,
    obj_weights, y_temperature, pixel_mask): host array}.  Every other label set is -1 (unlabelled); the other slots of the other
    regions stay 0 (a kernel reading another temperature slot gives NaN)."""
    raw = ws.view(torch.uint8)
    nbytes = ws.numel() * ws.element_size()
    for name, a in inputs.items():
        off = L.workspace_offset(cd, model, name)
        if name == "labels":
            n = 4 * L.LABEL_SLOTS * ((cd.B + 3) // 4 * 4)
            assert off + n <= nbytes
            raw[off:off + n].fill_(255)
        h = torch.from_numpy(np.ascontiguousarray(a, INPUT_DTYPES.get(name, np.float32)).reshape(-1).view(np.uint8))
        assert off + h.numel() <= nbytes, (name, off, h.numel(), nbytes)
        raw[off:off + h.numel()].copy_(h)


def hip_step(model, d: O.Dims, flat, x, eps, u, seed=0, step=0, want_masks=False, alloc=None, flags=0, row0=0, mask_rows=None,
             inputs=None, want_ws=False):
    """One gmvae_step under sched_flags `flags` at row0 (in-kernel noise where eps / u is None).  Returns (grads_sum[P_pad]
    float64 numpy, tail[8]) (+ the step's ReLU masks with want_masks: mask_rows = the rows per example of the per-sample nets,
    d.S by default, S K with y summed out) (+ the workspace as a float32 device tensor and the dims with want_ws).  inputs:
    write_inputs' mapping.  The alloc= arena form takes the first nine arguments only."""
    if alloc is not None:
        assert not flags and not row0 and mask_rows is None and inputs is None and not want_ws
        return _hip_step_in(alloc, model, d, flat, x, eps, u, seed, step, want_masks)
    B = x.shape[0]
    cd = dims_of(d, B)
    cd.sched_flags, cd.row0 = flags, row0
    P, _ = L.param_count(cd, model)
    params = dev(flat, torch.float32)
    xd = dev(x, torch.uint8)
    ed = None if eps is None else dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
    ws = workspace(cd, model)
    if inputs:
        write_inputs(ws, cd, model, inputs)
    rc = L.lib.gmvae_step(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws),
                          seed, step, None, L.current_stream())
    L.check(rc, "gmvae_step")
    torch.cuda.synchronize()
    g = grads.cpu().numpy().astype(np.float64)
    out = (g[:P], g[P:])
    if want_masks:
        out += (device_masks(ws, cd, model, dataclasses.replace(d, S=mask_rows or d.S), B),)
    return out + ((ws, cd) if want_ws else ())


def hip_forward(model, d: O.Dims, flat, x, eps, u, want_rows=True, alloc=None):
    if alloc is not None:
        o = forward_in(alloc, model, d, flat, x, eps, u)
        return o["tail"], o["rows"], o["z"], o["y"], o["logits"]
    B = x.shape[0]
    cd = dims_of(d, B)
    R = B * d.S
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    ed = None if eps is None else dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    tail = torch.zeros(L.TAIL, dtype=torch.float32, device="cuda")
    rows = torch.zeros(R, 4, dtype=torch.float32, device="cuda")
    z = torch.zeros(R, d.L, dtype=torch.float32, device="cuda")
    y = torch.zeros(R, d.K, dtype=torch.float32, device="cuda")
    lg = torch.zeros(B, d.K, dtype=torch.float32, device="cuda")
    ws = workspace(cd, model)
    rc = L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail),
                             L.ptr(rows), L.ptr(z), L.ptr(y), L.ptr(lg), L.ptr(ws), 0, 0, L.current_stream())
    L.check(rc, "gmvae_forward")
    torch.cuda.synchronize()
    return tail.cpu().numpy(), rows.cpu().numpy(), z.cpu().numpy(), y.cpu().numpy(), lg.cpu().numpy()


def forward_call(model, d: O.Dims, flat, x, S, eps=None, u=None, row0=0, flags=0, seed=0, step=0, logits=False, alloc=None):
    """gmvae_forward at S samples under sched_flags `flags` (in-kernel noise when eps is None): (tail [8], rows [R, 4], logits
    [B, K] or None) as numpy, R = B S rows, B S K with y summed out.  Every output starts as NaN."""
    if alloc is not None:
        o = forward_in(alloc, model, dataclasses.replace(d, S=S), flat, x, eps, u, row0, flags, seed, step,
                       ("rows", "logits") if logits else ("rows",))
        return o["tail"], o["rows"], o.get("logits")
    B = x.shape[0]
    cd = dims_of(dataclasses.replace(d, S=S), B)
    cd.row0, cd.sched_flags = row0, flags
    R = B * S * (d.K if flags & (L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW) else 1)
    ws = workspace(cd, model)
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    rows = torch.full((R, 4), float("nan"), device="cuda")
    lg = torch.full((B, d.K), float("nan"), device="cuda") if logits else None
    xd, params = dev(x, torch.uint8), dev(flat, torch.float32)          # (held until the kernels have run)
    ed = None if eps is None else dev(eps, torch.float32)
    ud = None if u is None else dev(u, torch.float32)
    rc = L.lib.gmvae_forward(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail), L.ptr(rows), None,
                             None, L.ptr(lg), L.ptr(ws), seed, step, L.current_stream())
    L.check(rc, "gmvae_forward")
    torch.cuda.synchronize()
    return tail.cpu().numpy(), rows.cpu().numpy(), None if lg is None else lg.cpu().numpy()


# the chunked importance-sampling evaluators (include/gmvae_hip.h gmvae_<kind>): the names of their outputs, in the C signature's order
CHUNKED_OUTPUTS = {"iw_bound": ("bound", "mean_logw"), "iw_bound_enum_y": ("bound", "mean_logw"),
                   "posterior_y": ("log_joint", "log_post", "stats"), "posterior_component": ("log_joint", "log_post", "stats")}


def chunked_call(kind, model, d: O.Dims, flat, x, n, chunk, row0=0, flags=0, seed=0, step=0, omit=(), alloc=None):
    """One gmvae_<kind> call at n samples in passes of `chunk`: dict of its outputs (CHUNKED_OUTPUTS; bound and mean_logw [B],
    log_joint and log_post [B, K], stats [B, 4]) and tail [8] as numpy.  Every output starts as NaN; the ones named in `omit`
    are passed as NULL and left out."""
    if alloc is not None:
        return chunked_in(alloc, kind, model, d, flat, x, n, chunk, row0, flags, seed, step, omit)
    B = x.shape[0]
    cd = dims_of(dataclasses.replace(d, S=chunk), B)
    cd.row0, cd.sched_flags = row0, flags
    ws = torch.zeros(getattr(L, f"{kind}_workspace_bytes")(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    shape = {"bound": (B,), "mean_logw": (B,), "log_joint": (B, d.K), "log_post": (B, d.K), "stats": (B, 4)}
    out = {k: None if k in omit else torch.full(shape[k], float("nan"), device="cuda") for k in CHUNKED_OUTPUTS[kind]}
    out["tail"] = torch.full((L.TAIL,), float("nan"), device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    rc = getattr(L.lib, f"gmvae_{kind}")(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, *(L.ptr(t) for t in out.values()),
                                         L.ptr(ws), seed, step, L.current_stream())
    L.check(rc, f"gmvae_{kind}")
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items() if t is not None}


def lse(v, axis=None):
    """logsumexp in fp64 over `axis` (everything by default)."""
    v = np.asarray(v, np.float64)
    m = v.max(axis=axis, keepdims=True)
    return np.squeeze(m + np.log(np.exp(v - m).sum(axis=axis, keepdims=True)), axis=axis)


def _L():
    """The ctypes binding (gmvae_amd._lib), for the test modules that reach it through a call."""
    return L


def grad_errs(model, d, gs, g, B):
    """[(tensor name, max |gs / B - g| / max(max |g|, 1e-6))]: a step's gradient sums gs [P] against the statement's g."""
    lay, _, _ = O.param_layout(model, d)
    out = []
    for name, shape, off in lay:
        n = int(np.prod(shape))
        got, ref = gs[off:off + n].reshape(shape) / B, g[name]
        out.append((name, np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)))
    return out


def tail_gates(what, tail, B, Cc, rtol=1e-4):
    """The step's tail[0..4] against the statement's batch means: the loss and nll at rtol relative, kl and nent at rtol of
    max(|.|, 1) -- each term relative to itself (compare_step's reasons)."""
    print(f"{what}: tail {tail.tolist()} ref loss {Cc['loss']} nll {Cc['nll']} kl {Cc['kl']} nent {Cc['nent']}")
    print(f"{what}: rel err loss {abs(tail[0] / B - Cc['loss']) / abs(Cc['loss']):.3e}")
    assert tail[4] == B
    assert abs(tail[0] / B - Cc["loss"]) <= rtol * abs(Cc["loss"]), (what, tail[0] / B, Cc["loss"])
    assert abs(tail[1] / B - Cc["nll"]) <= rtol * abs(Cc["nll"]), (what, tail[1] / B, Cc["nll"])
    assert abs(tail[2] / B - Cc["kl"]) <= rtol * max(abs(Cc["kl"]), 1.0), (what, tail[2] / B, Cc["kl"])
    assert abs(tail[3] / B - Cc["nent"]) <= rtol * max(abs(Cc["nent"]), 1.0), (what, tail[3] / B, Cc["nent"])


def check_grads(what, model, d, gs, g, B, masks, pre, recompute, rtol=1e-4):
    """Every gradient tensor at rtol of its own max.  A tensor outside it under ReLU: the device's ReLU took another side than
    fp64 somewhere?  Legitimate only at units that are numerically zero in fp64 (check_masks asserts it); recompute(masks) then
    gives the statement's g under the device's subgradients and the gates apply to that.  Returns the errors."""
    errs = grad_errs(model, d, gs, g, B)
    if max(e for _, e in errs) > rtol and getattr(d, "act", "relu") == "relu":
        if check_masks(masks, pre, what):
            errs = grad_errs(model, d, gs, recompute(masks), B)
    for name, err in errs:
        print(f"{what} {name}: rel-to-max err {err:.3e}")
    for name, err in errs:
        assert err <= rtol, f"{what} {name}: rel-to-max err {err:.3e}"
    return errs


def need_rccl():
    """The one narrow precondition of the one-rank communicator tests, decided before any work: the RCCL shared library itself
    loads in this process.  Everything after it -- the project's own communicator code included -- fails the test if it fails."""
    import pytest
    try:
        C.CDLL(L.rccl_path().decode())
    except OSError as e:
        pytest.skip(f"the RCCL shared library does not load here: {e}")


def drop_comm(b):
    """The end of a one-rank communicator test: the engine's graphs, then its communicator."""
    torch.cuda.synchronize()
    b.drop_graphs()
    if getattr(b, "_comm", None):
        L.check(L.lib.gmvae_comm_destroy(b._comm), "gmvae_comm_destroy")
        b._comm = None


MARGINS = []      # (what, worst error / its gate) of every compare_step call: tests/test_hip_parity.py prints the maxima


def compare_step(model, d, p, x, eps, u, loss_rtol=1e-4, grad_rtol=1e-4, alloc=None):
    """HIP step vs the fp64 oracle on identical (params, x, eps, u).  Gates: the ELBO at loss_rtol
    relative (north_star's 1e-4), and EACH term relative to ITSELF -- |d nll| <= 1e-4 |nll|, |d kl| <= 1e-4 max(|kl|, 1),
    |d nent| <= 1e-4 max(|nent|, 1) -- so that the O(1-10) kl and entropy terms cannot hide inside the budget of an
    O(500) loss; every gradient tensor at grad_rtol of its own max.

    ReLU has no derivative at 0, and an fp32 pre-activation that is zero to within rounding can land on the other side than
    the fp64 one (one unit in ~10^5 at these sizes): the oracle takes the device's subgradient there -- and only there:
    check_masks asserts that every unit whose mask differs is numerically zero in fp64 -- so that any seed runs inside the
    same gates (tests/test_timed_path.py does the same over trajectories)."""
    B = x.shape[0]
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))            # the values the GPU actually sees
    Cc, g = O.loss_and_grads(model, d, p32, x, eps, u, np.float64)
    gs, tail, masks = hip_step(model, d, flat, x, eps, u, want_masks=True, alloc=alloc)
    assert tail[4] == B
    loss = tail[0] / B
    assert abs(loss - Cc["loss"]) <= loss_rtol * abs(Cc["loss"]), (loss, Cc["loss"])
    terms = {"nll": (tail[1] / B, Cc["nll"], loss_rtol * abs(Cc["nll"])),
             "kl": (tail[2] / B, Cc["kl"], 1e-4 * max(abs(Cc["kl"]), 1.0)),
             "nent": (tail[3] / B, Cc["nent"], 1e-4 * max(abs(Cc["nent"]), 1.0))}
    MARGINS.append(("loss", abs(loss - Cc["loss"]) / (loss_rtol * abs(Cc["loss"]))))
    for nm, (got, ref, gate) in terms.items():
        MARGINS.append((nm, abs(got - ref) / gate))
        assert abs(got - ref) <= gate, f"{nm}: {got} vs {ref} (gate {gate:.2e})"
    who = [k for k, v in O.MODEL_NAMES.items() if v == model][0]
    errs = check_grads(f"{who} B={B} D={d.D} L={d.L} K={d.K} H={d.hidden} S={d.S}", model, d, gs, g, B, masks, Cc["pre"],
                       lambda m: O.loss_and_grads(model, d, p32, x, eps, u, np.float64, relu_masks=m)[1], grad_rtol)
    MARGINS.extend(("grad S>1" if d.S > 1 else "grad", err / grad_rtol) for _, err in errs)
    return loss, max(err for _, err in errs)
