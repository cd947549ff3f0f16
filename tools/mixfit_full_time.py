"""Time of gmvae_amd.mixfit with covariance="full" (include/gmvae_hip.h gmvae_mixfit_full_*: a full-covariance Gaussian mixture fitted
by EM on the device) at N codes of L dimensions and K components -- the whole fit() call from a given init, one iteration (by
difference against a 0-iteration call), and one assign pass -- against a chunked torch implementation of the same statement on the
same device: torch.linalg.cholesky, solve_triangular and einsum in fp64, the centred sums accumulated across chunks, no host
synchronisation inside.  The diagonal fit's time per iteration is printed for context.  Device events after a warm-up, alternating
rounds:
    python tools/mixfit_full_time.py [N] [L] [K] [rounds] [iters] [torch_iters] [chunk]
(default N = 60,000, L = 64, K = 10, 3 rounds, 20 iterations, 3 torch iterations, chunks of 4096 rows).  Prints one JSON line."""
import json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import mixfit

a = sys.argv[1:]
N, Lz, K, rounds, iters, titers, CHUNK = (int(v) for v in (a[:7] + ["60000", "64", "10", "3", "20", "3", "4096"][len(a[:7]):]))
REG, EPS0 = 1e-6, 10 * 2.0 ** -52
rng = np.random.default_rng(0)
centers = rng.normal(0, 3, (K, Lz))
mix = rng.normal(0, 1, (K, Lz, Lz)) / math.sqrt(Lz) + np.eye(Lz)[None]          # clusters that are not axis-aligned
lab = np.arange(N) % K
codes = torch.from_numpy((centers[lab] + np.einsum("nd,ned->ne", rng.normal(0, 1, (N, Lz)), mix[lab])).astype(np.float32)).cuda()
init = (torch.full((K,), -math.log(K), device="cuda"), codes[:K].clone(), torch.eye(Lz, device="cuda").expand(K, Lz, Lz).contiguous())
init_diag = (init[0], init[1], torch.ones(K, Lz, device="cuda"))


@torch.no_grad()
def torch_iteration(z, logw, mu, cov):
    dev = z.device
    C = torch.linalg.cholesky(cov.double())
    c = logw.double() - C.diagonal(dim1=1, dim2=2).log().sum(dim=1) - 0.5 * Lz * math.log(2 * math.pi)
    R = torch.zeros(K, dtype=torch.float64, device=dev)
    S1 = torch.zeros(K, Lz, dtype=torch.float64, device=dev)
    S2 = torch.zeros(K, Lz, Lz, dtype=torch.float64, device=dev)
    ll = torch.zeros((), dtype=torch.float64, device=dev)
    for r0 in range(0, z.shape[0], CHUNK):
        dz = z[r0:r0 + CHUNK].double()[None, :, :] - mu.double()[:, None, :]                      # [K, n, L]
        y = torch.linalg.solve_triangular(C, dz.transpose(1, 2), upper=False)                    # [K, L, n]
        l = (c[:, None] - 0.5 * (y * y).sum(dim=1)).t()                                          # [n, K]
        lse = torch.logsumexp(l, dim=1)
        r = (l - lse[:, None]).float().exp().double()
        R += r.sum(dim=0)
        rd = r.t()[:, :, None] * dz
        S1 += rd.sum(dim=1)
        S2 += torch.einsum("knd,kne->kde", rd, dz)
        ll += lse.sum()
    Rp = R + EPS0
    m = S1 / Rp[:, None]
    cov2 = S2 / Rp[:, None, None] - m[:, :, None] * m[:, None, :]
    d = torch.arange(Lz, device=dev)
    cov2[:, d, d] = cov2[:, d, d].clamp_min(0.0) + REG
    return (Rp / Rp.sum()).log().float(), (mu.double() + m).float(), cov2.float(), ll / z.shape[0]


def torch_fit(n):
    logw, mu, cov = (t.clone() for t in init)
    for _ in range(n):
        logw, mu, cov, _ = torch_iteration(codes, logw, mu, cov)
    return logw, mu, cov


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


fitted = mixfit.fit(codes, K, n_iter=iters, init=init, covariance="full")
fns = {"hip_fit": lambda: mixfit.fit(codes, K, n_iter=iters, init=init, covariance="full"),
       "hip_fit_0_iters": lambda: mixfit.fit(codes, K, n_iter=0, init=init, covariance="full"),
       "hip_assign": lambda: mixfit.assign(codes, fitted),
       "diag_fit": lambda: mixfit.fit(codes, K, n_iter=iters, init=init_diag),
       "diag_fit_0_iters": lambda: mixfit.fit(codes, K, n_iter=0, init=init_diag)}
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
       "workspace_bytes": mixfit.full_workspace_bytes(N, Lz, K)}
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
# fit() = the start + iters iterations (three launches each) + one closing assign (two launches): the iteration's share by difference
out["hip_iteration_ms"] = round((out["hip_fit_ms"] - out["hip_fit_0_iters_ms"]) / max(iters, 1), 4)
out["diag_iteration_ms"] = round((out["diag_fit_ms"] - out["diag_fit_0_iters_ms"]) / max(iters, 1), 4)
fma = N * K * Lz * Lz * 1.5                                # N K L^2 (1/2 for the triangular product, 1 for the S2 sum as counted dense)
if out["hip_iteration_ms"] > 0:
    out["fp64_fma_per_s_per_iteration"] = round(fma / (out["hip_iteration_ms"] * 1e-3))
    out["fraction_of_vector_fp64_peak"] = round(fma / (out["hip_iteration_ms"] * 1e-3) / (78.6e12 / 2), 4)      # 78.6 TFLOP/s = 39.3 T fma/s
out.update(loglik=float(fitted["loglik"]), loglik_first=float(fitted["loglik_history"][0]) if iters else None,
           info=fitted["info"].tolist(), finite=bool(all(torch.isfinite(fitted[k]).all() for k in ("logw", "mu", "cov"))))
if titers > 0:
    out["torch_iteration_ms"] = round(out["torch_iterations_ms"] / titers, 3)
    out["torch_over_hip_iteration"] = round(out["torch_iteration_ms"] / out["hip_iteration_ms"], 1) if out["hip_iteration_ms"] > 0 else None
    tl, tm, tc = torch_fit(titers)
    h = mixfit.fit(codes, K, n_iter=titers, init=init, covariance="full")
    out["max_diff_vs_torch"] = {"logw": float((tl - h["logw"]).abs().max()), "mu": float((tm - h["mu"]).abs().max()),
                                "cov": float((tc - h["cov"]).abs().max())}
print(json.dumps(out), flush=True)
