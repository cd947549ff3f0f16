"""Time of gmvae_amd.mixfit (include/gmvae_hip.h gmvae_mixfit_*: a diagonal Gaussian mixture fitted by EM on the device) at N codes
of L dimensions and K components -- the whole fit() call from a given init, one iteration (by difference against a 0-iteration
call), and one assign pass -- against a chunked torch implementation of the same statement on the same device: the E-step in
[chunk, K, L] blocks with fp64 differences (as the HIP path), the centred sums accumulated in fp64 across chunks, no host
synchronisation inside.  Device events after a warm-up, alternating rounds:
    python tools/mixfit_time.py [N] [L] [K] [rounds] [iters] [torch_iters] [chunk]
(default N = 60,000, L = 64, K = 10, 3 rounds, 100 iterations, 10 torch iterations, chunks of 4096 rows).  Prints one JSON line."""
import json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import mixfit

a = sys.argv[1:]
N, Lz, K, rounds, iters, titers, CHUNK = (int(v) for v in (a[:7] + ["60000", "64", "10", "3", "100", "10", "4096"][len(a[:7]):]))
REG, EPS0 = 1e-6, 10 * 2.0 ** -52
rng = np.random.default_rng(0)
centers = rng.normal(0, 3, (K, Lz))
codes = torch.from_numpy((centers[np.arange(N) % K] + rng.normal(0, 1, (N, Lz))).astype(np.float32)).cuda()
init = (torch.full((K,), -math.log(K), device="cuda"), codes[:K].clone(), torch.ones(K, Lz, device="cuda"))      # one code per cluster


@torch.no_grad()
def torch_estep(z, logw, mu, sigma):
    """(lse [n], log_resp [n, K]) of a chunk, fp64."""
    t = (z.double()[:, None, :] - mu.double()[None]) / sigma.double()[None]
    l = logw.double()[None] - 0.5 * (t * t).sum(dim=2) - sigma.double().log().sum(dim=1)[None] - 0.5 * z.shape[1] * math.log(2 * math.pi)
    lse = torch.logsumexp(l, dim=1)
    return lse, l - lse[:, None]


@torch.no_grad()
def torch_iteration(z, logw, mu, sigma):
    R = torch.zeros(K, dtype=torch.float64, device=z.device)
    S1, S2 = torch.zeros(K, Lz, dtype=torch.float64, device=z.device), torch.zeros(K, Lz, dtype=torch.float64, device=z.device)
    ll = torch.zeros((), dtype=torch.float64, device=z.device)
    for r0 in range(0, z.shape[0], CHUNK):
        zc = z[r0:r0 + CHUNK]
        lse, lr = torch_estep(zc, logw, mu, sigma)
        r = lr.float().exp().double()
        dz = zc.double()[:, None, :] - mu.double()[None]
        R += r.sum(dim=0)
        S1 += (r[:, :, None] * dz).sum(dim=0)
        S2 += (r[:, :, None] * dz * dz).sum(dim=0)
        ll += lse.sum()
    Rp = R + EPS0
    m = S1 / Rp[:, None]
    var = (S2 / Rp[:, None] - m * m).clamp_min(0.0)
    return (Rp / Rp.sum()).log().float(), (mu.double() + m).float(), (var + REG).sqrt().float(), ll / z.shape[0]


def torch_fit(n):
    logw, mu, sigma = (t.clone() for t in init)
    for _ in range(n):
        logw, mu, sigma, _ = torch_iteration(codes, logw, mu, sigma)
    return logw, mu, sigma


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


fitted = mixfit.fit(codes, K, n_iter=iters, init=init)
fns = {"hip_fit": lambda: mixfit.fit(codes, K, n_iter=iters, init=init),
       "hip_fit_0_iters": lambda: mixfit.fit(codes, K, n_iter=0, init=init),
       "hip_assign": lambda: mixfit.assign(codes, fitted)}
if titers > 0:
    fns["torch_iterations"] = lambda: torch_fit(titers)
for fn in fns.values():                                  # warm-up: code objects, the caching allocator
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in fns}
for r in range(rounds):                                  # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k]))
out = {"N": N, "L": Lz, "K": K, "rounds": rounds, "iters": iters, "torch_iters": titers, "torch_chunk": CHUNK,
       "workspace_bytes": mixfit.workspace_bytes(N, Lz, K)}
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
# fit() = the start + iters iterations (two launches each) + one closing assign pass: the iteration's share by difference
out["hip_iteration_ms"] = round((out["hip_fit_ms"] - out["hip_fit_0_iters_ms"]) / max(iters, 1), 4)
if out["hip_iteration_ms"] > 0:
    out["codes_bytes_per_s_per_iteration"] = round(N * Lz * 4 / (out["hip_iteration_ms"] * 1e-3))
out.update(loglik=float(fitted["loglik"]), loglik_first=float(fitted["loglik_history"][0]) if iters else None,
           finite=bool(all(torch.isfinite(fitted[k]).all() for k in ("logw", "mu", "sigma"))))
if titers > 0:
    out["torch_iteration_ms"] = round(out["torch_iterations_ms"] / titers, 3)
    out["torch_over_hip_iteration"] = round(out["torch_iteration_ms"] / out["hip_iteration_ms"], 1) if out["hip_iteration_ms"] > 0 else None
    tl, tm, ts = torch_fit(titers)
    h = mixfit.fit(codes, K, n_iter=titers, init=init)
    out["max_diff_vs_torch"] = {"logw": float((tl - h["logw"]).abs().max()), "mu": float((tm - h["mu"]).abs().max()),
                                "sigma": float(((ts - h["sigma"]) / h["sigma"]).abs().max())}
print(json.dumps(out), flush=True)
