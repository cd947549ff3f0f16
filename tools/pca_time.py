"""Time of gmvae_amd.pca (include/gmvae_hip.h gmvae_pca_*, gmvae_sym_eigh) -- fit and transform at N x 64 -> k = 64 and at N x 784 ->
k = 50, eigh at n = 128 -- against a chunked torch fp64 implementation of the same statement on the same device: the fp64-centred
x.T @ x in row chunks, torch.linalg.eigh (on the device where it runs there, else on the host: the output says which), an fp64 matmul
for the transform.  The covariance pass's time by difference: the fit with one sweep (D <= 128) or with no iteration and one sweep
(D > 128) is the pass plus a known remainder, which the same differences give.  Device events after a warm-up, alternating rounds:
    python tools/pca_time.py [N] [rounds] [chunk]
(default N = 60,000, 5 rounds, chunks of 8192 rows).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import pca

a = sys.argv[1:]
N, rounds, CHUNK = (int(v) for v in (a[:3] + ["60000", "5", "8192"][len(a[:3]):]))
FP64_MATRIX_FLOPS = 78.6e12      # the MI355X's fp64 matrix peak (public specification)
CASES = [(64, 64), (784, 50)]


def data(D):
    rng = np.random.default_rng(D)
    basis = np.linalg.qr(rng.standard_normal((D, D)))[0]
    return torch.from_numpy(((rng.standard_normal((N, D)) * np.sqrt(0.97 ** np.arange(D))) @ basis.T + 1.0).astype(np.float32)).cuda()


@torch.no_grad()
def torch_cov(x):
    mu = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    for r0 in range(0, N, CHUNK):
        mu += x[r0:r0 + CHUNK].double().sum(dim=0)
    mu /= N
    C = torch.zeros(x.shape[1], x.shape[1], dtype=torch.float64, device=x.device)
    for r0 in range(0, N, CHUNK):
        xc = x[r0:r0 + CHUNK].double() - mu
        C += xc.T @ xc
    return mu, C / (N - 1)


EIGH_ON = "device"
try:
    torch.linalg.eigh(torch.eye(4, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
except Exception:      # no device solver in this build: the host's
    EIGH_ON = "host"


@torch.no_grad()
def torch_eigh(A):
    if EIGH_ON == "device":
        return torch.linalg.eigh(A)
    w, V = torch.linalg.eigh(A.cpu())
    return w.to(A.device), V.to(A.device)


@torch.no_grad()
def torch_fit(x, k):
    mu, C = torch_cov(x)
    w, V = torch_eigh(C)
    return mu, V[:, -k:].flip(1).T.contiguous(), w[-k:].flip(0)


@torch.no_grad()
def torch_transform(x, mu, comp):
    out = torch.empty(N, comp.shape[0], dtype=torch.float32, device=x.device)
    for r0 in range(0, N, CHUNK):
        out[r0:r0 + CHUNK] = ((x[r0:r0 + CHUNK].double() - mu) @ comp.T).float()
    return out


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


out = {"N": N, "rounds": rounds, "torch_chunk": CHUNK, "torch_eigh_on": EIGH_ON, "n_sweeps": pca.N_SWEEPS, "n_iter": pca.N_ITER}
fns, keep = {}, {}
for D, k in CASES:
    x = data(D)
    f = pca.fit(x, n_components=k)
    tmu, tcomp, tw = torch_fit(x, k)
    keep[D] = (x, f, tmu, tcomp, tw)
    fns[f"hip_fit_{D}"] = lambda x=x, k=k: pca.fit(x, n_components=k)
    fns[f"hip_fit_{D}_one_sweep"] = lambda x=x, k=k: pca.fit(x, n_components=k, n_iter=0, n_sweeps=1)
    fns[f"hip_fit_{D}_two_sweeps"] = lambda x=x, k=k: pca.fit(x, n_components=k, n_iter=0, n_sweeps=2)
    fns[f"hip_transform_{D}"] = lambda x=x, f=f: pca.transform(x, f)
    fns[f"torch_cov_{D}"] = lambda x=x: torch_cov(x)
    fns[f"torch_fit_{D}"] = lambda x=x, k=k: torch_fit(x, k)
    fns[f"torch_transform_{D}"] = lambda x=x, tmu=tmu, tcomp=tcomp: torch_transform(x, tmu, tcomp)
A = keep[64][1]["components"].T @ torch.diag(torch.linspace(1.0, 2.0, 64, dtype=torch.float64, device="cuda")) @ keep[64][1]["components"]
A128 = torch.block_diag(A, 0.5 * A) + 0.01
A128 = 0.5 * (A128 + A128.T)
fns["hip_eigh_128"] = lambda: pca.eigh(A128)
fns["hip_eigh_128_one_sweep"] = lambda: pca.eigh(A128, n_sweeps=1)
fns["torch_eigh_128"] = lambda: torch_eigh(A128)
for fn in fns.values():                                  # warm-up: code objects, the caching allocator, the libraries' choices
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in fns}
for r in range(rounds):                                  # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k]))
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
out["hip_sweep_128_ms"] = round((out["hip_eigh_128_ms"] - out["hip_eigh_128_one_sweep_ms"]) / (pca.N_SWEEPS - 1), 4)
for D, k in CASES:
    x, f, tmu, tcomp, tw = keep[D]
    # the fit with one sweep = the moments, the covariance pass and its fold, the copy of V0 and one product C V (D > 128), one sweep
    # and the outputs; a sweep by the difference of two; what is left is charged to the covariance pass (an upper bound on it)
    sweep = out[f"hip_fit_{D}_two_sweeps_ms"] - out[f"hip_fit_{D}_one_sweep_ms"]
    cov = out[f"hip_fit_{D}_one_sweep_ms"] - sweep
    out[f"hip_cov_pass_{D}_ms"] = round(cov, 3)
    out[f"hip_cov_share_of_fit_{D}"] = round(cov / out[f"hip_fit_{D}_ms"], 3)
    # the lower triangle in 64 x 64 macro-blocks is what the pass multiplies: 2 flops per row, per entry
    nmb = (D + 63) // 64
    flops = 2.0 * N * (nmb * (nmb + 1) // 2) * 64 * 64
    out[f"hip_cov_fp64_matrix_share_{D}"] = round(flops / (cov * 1e-3) / FP64_MATRIX_FLOPS, 4) if cov > 0 else None
    out[f"torch_over_hip_fit_{D}"] = round(out[f"torch_fit_{D}_ms"] / out[f"hip_fit_{D}_ms"], 2)
    out[f"torch_over_hip_transform_{D}"] = round(out[f"torch_transform_{D}_ms"] / out[f"hip_transform_{D}_ms"], 2)
    out[f"max_diff_vs_torch_{D}"] = {"explained_variance": float((f["explained_variance"] - tw).abs().max()),
                                     "components": float((f["components"].abs() - tcomp.abs()).abs().max()),
                                     "transform": float((pca.transform(x, f).abs() - torch_transform(x, tmu, tcomp).abs()).abs().max()),
                                     "residual_max": float(f["residual"].max()), "offdiag": float(f["offdiag"]), "info": int(f["info"])}
out["torch_over_hip_eigh_128"] = round(out["torch_eigh_128_ms"] / out["hip_eigh_128_ms"], 3)
print(json.dumps(out), flush=True)
