"""Time of gmvae_amd.sinkhorn (include/gmvae_hip.h gmvae_sinkhorn: the debiased Sinkhorn divergence on the device) at n + n rows of D
dimensions and T iterations -- the library call on a schedule already on the device -- against two fp64 torch implementations of the
same statement on the same device: (a) chunked, the costs recomputed in [chunk, n] blocks from the centred expanded square in every
softmin, nothing n^2 stored; (b) stored, the three cost matrices kept in fp64.  No host synchronisation inside any of them.  Device
events after a warm-up, alternating rounds:
    python tools/sinkhorn_time.py [n] [D] [T] [rounds] [chunk]
(default n = 10,000, D = 64, T = 200, 5 rounds, chunks of 2048 rows).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import sinkhorn, twosample

a = sys.argv[1:]
n, D, T, rounds, CHUNK = (int(v) for v in (a[:5] + ["10000", "64", "200", "5", "2048"][len(a[:5]):]))
g = torch.Generator(device="cuda").manual_seed(0)
if D == 784:      # binary pixels at two densities
    x = (torch.rand(n, D, device="cuda", generator=g) < 0.30).float()
    y = (torch.rand(n, D, device="cuda", generator=g) < 0.31).float()
else:             # codes: two Gaussians a little apart
    x = torch.randn(n, D, device="cuda", generator=g)
    y = torch.randn(n, D, device="cuda", generator=g) * 1.05 + 0.05
z = torch.cat([x, y])
eps = sinkhorn.schedule(z, T)
zc = z.double() - z.double().mean(dim=0)
xc, yc = zc[:n], zc[n:]
logw = torch.full((n,), -float(np.log(n)), dtype=torch.float64, device="cuda")


def cost_block(u, v, r0, r1, same):
    c = (0.5 * ((u[r0:r1] * u[r0:r1]).sum(dim=1)[:, None] + (v * v).sum(dim=1)[None, :]) - u[r0:r1] @ v.t()).clamp_min_(0.0)
    if same:
        c[torch.arange(r1 - r0, device="cuda"), torch.arange(r0, r1, device="cuda")] = 0.0
    return c


def softmin_chunked(u, v, same, h, e):
    out = torch.empty(u.shape[0], dtype=torch.float64, device="cuda")
    for r0 in range(0, u.shape[0], CHUNK):
        r1 = min(u.shape[0], r0 + CHUNK)
        out[r0:r1] = -e * torch.logsumexp(logw[None, :] + (h[None, :] - cost_block(u, v, r0, r1, same)) / e, dim=1)
    return out


def softmin_stored(c, h, e):
    return -e * torch.logsumexp(logw[None, :] + (h[None, :] - c) / e, dim=1)


@torch.no_grad()
def run(sm_xy, sm_yx, sm_xx, sm_yy):
    f, g_, p, q = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(4))
    for t in range(T):
        e = eps[t]
        f = sm_xy(g_, e)
        p, q = 0.5 * (p + sm_xx(p, e)), 0.5 * (q + sm_yy(q, e))
        g_ = sm_yx(f, e)
        p, q = 0.5 * (p + sm_xx(p, e)), 0.5 * (q + sm_yy(q, e))
    e = eps[T]
    f1, p1, q1 = sm_xy(g_, e), sm_xx(p, e), sm_yy(q, e)
    return (f1 - p1).mean() + (g_ - q1).mean(), torch.expm1((f - f1) / e).abs().max()


def torch_chunked():
    return run(lambda h, e: softmin_chunked(xc, yc, False, h, e), lambda h, e: softmin_chunked(yc, xc, False, h, e),
               lambda h, e: softmin_chunked(xc, xc, True, h, e), lambda h, e: softmin_chunked(yc, yc, True, h, e))


def torch_stored():
    cxy, cxx, cyy = cost_block(xc, yc, 0, n, False), cost_block(xc, xc, 0, n, True), cost_block(yc, yc, 0, n, True)
    cyx = cxy.t()
    return run(lambda h, e: softmin_stored(cxy, h, e), lambda h, e: softmin_stored(cyx, h, e), lambda h, e: softmin_stored(cxx, h, e),
               lambda h, e: softmin_stored(cyy, h, e))


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


fns = {"hip": lambda: sinkhorn.solve(x, y, eps), "torch_chunked": torch_chunked, "torch_stored": torch_stored}
got = sinkhorn.solve(x, y, eps)                          # (also the warm-up: code objects, the caching allocator, rocBLAS's choices)
ref_c, ref_s = torch_chunked(), torch_stored()
torch.cuda.synchronize()
out = {"n": n, "m": n, "D": D, "T": T, "rounds": rounds, "torch_chunk": CHUNK, "workspace_bytes": sinkhorn.workspace_bytes(n, n, D)}
for k, fn in fns.items():
    out[f"{k}_peak_bytes"] = peak(fn)
ms = {k: [] for k in fns}
for r in range(rounds):                                  # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k]))
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
out["hip_ms_per_pass"] = round(out["hip_ms"] / (2 * T + 1), 4)      # a pass: a half-step's three softmins
out["torch_chunked_over_hip"] = round(out["torch_chunked_ms"] / out["hip_ms"], 3)
out["torch_stored_over_hip"] = round(out["torch_stored_ms"] / out["hip_ms"], 3)
cscale = (0.5 * twosample.rms_distance(z) ** 2).item()
out["sinkhorn"], out["cscale"], out["marginal_err"] = got["sinkhorn"].item(), cscale, got["marginal_err"].item()
out["diff_vs_torch_chunked_in_cscale"] = abs(got["sinkhorn"].item() - ref_c[0].item()) / cscale
out["diff_vs_torch_stored_in_cscale"] = abs(got["sinkhorn"].item() - ref_s[0].item()) / cscale
out["marginal_err_torch_stored"] = ref_s[1].item()
print(json.dumps(out), flush=True)
