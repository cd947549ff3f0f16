"""Time of gmvae_amd.linprobe (include/gmvae_hip.h gmvae_linprobe_*: softmax regression fitted by FISTA in Boehning's metric on the
device) at N codes of L dimensions and C classes -- the whole fit() call, one iteration (by difference against a 0-iteration call,
which is the set-up), and one predict pass -- against a chunked torch implementation of the same statement on the same device:
fp64 throughout, the logits and the gradient sums in [chunk, C] blocks accumulated across chunks, the metric by torch.linalg, no
host synchronisation inside.  Device events after a warm-up, alternating rounds:
    python tools/linprobe_time.py [N] [L] [C] [rounds] [iters] [torch_iters] [chunk]
(default N = 60,000, L = 64, C = 10, 3 rounds, 300 iterations, 20 torch iterations, chunks of 8192 rows).  Prints one JSON line."""
import json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import linprobe

a = sys.argv[1:]
N, Lz, C, rounds, iters, titers, CHUNK = (int(v) for v in (a[:7] + ["60000", "64", "10", "3", "300", "20", "8192"][len(a[:7]):]))
L2 = 1e-3
rng = np.random.default_rng(0)
centers = rng.normal(0, 2.0 / math.sqrt(Lz), (C, Lz))
y_np = (np.arange(N) % C).astype(np.int32)
codes = torch.from_numpy((centers[y_np] + rng.normal(0, 1, (N, Lz))).astype(np.float32)).cuda()
y_np[rng.random(N) < 0.3] = -1
labels = torch.from_numpy(y_np).cuda()


@torch.no_grad()
def torch_setup():
    w = ((labels >= 0) & (labels < C)).double()
    n = w.sum()
    x = codes.double()
    xbar = (w[:, None] * x).sum(dim=0) / n
    xc = (x - xbar) * w[:, None]
    A = 0.5 * (xc.T @ xc) / n + L2 * torch.eye(Lz, dtype=torch.float64, device=codes.device)
    return n, xbar, torch.cholesky_inverse(torch.linalg.cholesky(A))


@torch.no_grad()
def torch_fit(n_it):
    n, xbar, Ainv = torch_setup()
    ThW, Thb = torch.zeros(Lz, C, dtype=torch.float64, device="cuda"), torch.zeros(C, dtype=torch.float64, device="cuda")
    VW, Vb, t = ThW.clone(), Thb.clone(), 1.0
    for _ in range(n_it):
        GW, Gb = torch.zeros_like(VW), torch.zeros_like(Vb)
        for r0 in range(0, N, CHUNK):
            yc = labels[r0:r0 + CHUNK].long()
            w = ((yc >= 0) & (yc < C)).double()
            xc = codes[r0:r0 + CHUNK].double() - xbar
            p = torch.softmax(xc @ VW + Vb, dim=1)
            r = (p - torch.nn.functional.one_hot(yc.clamp(0, C - 1), C).double()) * w[:, None]
            GW += xc.T @ r
            Gb += r.sum(dim=0)
        GW = GW / n + L2 * VW
        nW, nb = VW - Ainv @ GW, Vb - 2.0 * Gb / n
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta, t = (t - 1.0) / t1, t1
        VW, Vb = nW + beta * (nW - ThW), nb + beta * (nb - Thb)
        ThW, Thb = nW, nb
    return ThW.float(), (Thb - xbar @ ThW).float()


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


fitted = linprobe.fit(codes, labels, C, l2=L2, n_iter=iters)
fns = {"hip_fit": lambda: linprobe.fit(codes, labels, C, l2=L2, n_iter=iters),
       "hip_fit_0_iters": lambda: linprobe.fit(codes, labels, C, l2=L2, n_iter=0),
       "hip_predict": lambda: linprobe.predict(codes, fitted)}
if titers > 0:
    fns["torch_iterations"] = lambda: torch_fit(titers)
    fns["torch_setup"] = torch_setup
for fn in fns.values():                                  # warm-up: code objects, the caching allocator
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in fns}
for r in range(rounds):                                  # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k]))
out = {"N": N, "L": Lz, "C": C, "rounds": rounds, "iters": iters, "torch_iters": titers, "torch_chunk": CHUNK,
       "workspace_bytes": linprobe.workspace_bytes(N, Lz, C)}
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
# fit() = the set-up launch + iters iterations (two launches each): the iteration's share by difference
out["hip_setup_ms"] = out["hip_fit_0_iters_ms"]
out["hip_iteration_ms"] = round((out["hip_fit_ms"] - out["hip_fit_0_iters_ms"]) / max(iters, 1), 4)
if out["hip_iteration_ms"] > 0:
    out["codes_bytes_per_s_per_iteration"] = round(N * Lz * 4 / (out["hip_iteration_ms"] * 1e-3))
sc = linprobe.score(codes, labels, fitted)
out.update(loss_first=float(fitted["loss_history"][0]) if iters else None, loss_last=float(fitted["loss_history"][-1]) if iters else None,
           grad_max=float(fitted["grad_max"]), info=int(fitted["info"]), accuracy=float(sc["accuracy"]),
           finite=bool(torch.isfinite(fitted["W"]).all() and torch.isfinite(fitted["b"]).all()))
if titers > 0:
    out["torch_iteration_ms"] = round((out["torch_iterations_ms"] - out["torch_setup_ms"]) / titers, 3)
    out["torch_over_hip_iteration"] = round(out["torch_iteration_ms"] / out["hip_iteration_ms"], 1) if out["hip_iteration_ms"] > 0 else None
    tW, tb = torch_fit(titers)
    h = linprobe.fit(codes, labels, C, l2=L2, n_iter=titers)
    out["max_diff_vs_torch"] = {"W": float((tW - h["W"]).abs().max()), "b": float((tb - h["b"]).abs().max()),
                                "max_W": float(h["W"].abs().max())}
print(json.dumps(out), flush=True)
