"""Time of gmvae_amd.twosample (include/gmvae_hip.h gmvae_mmd: the kernel two-sample test on the device) at n + n rows of D dimensions
and P splits -- the whole mmd_test() call (the seeded permutations drawn on the host and uploaded, the median bandwidth read back,
then the library call), the library call alone on splits already on the device (five launches under rbf, two under energy), and
the same at P = 1 (the Gram part; the permutation part by difference) -- against a chunked torch implementation of the same statement on the same device: fp64 throughout, the Gram matrix in
[chunk, N] blocks from the centred expanded square, each block multiplied into all P splits at once, no host synchronisation
inside.  Device events after a warm-up, alternating rounds:
    python tools/twosample_time.py [n] [D] [P] [rounds] [chunk] [kernel]
(default n = 10,000, D = 784, P = 1000, 9 rounds, chunks of 2048 rows, rbf).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import twosample

a = sys.argv[1:]
n, D, P, rounds, CHUNK = (int(v) for v in (a[:5] + ["10000", "784", "1000", "9", "2048"][len(a[:5]):]))
kernel = a[5] if len(a) > 5 else "rbf"
N = 2 * n
g = torch.Generator(device="cuda").manual_seed(0)
if D == 784:      # binary pixels at two densities
    x = (torch.rand(n, D, device="cuda", generator=g) < 0.30).float()
    y = (torch.rand(n, D, device="cuda", generator=g) < 0.31).float()
else:             # codes: two Gaussians a little apart
    x = torch.randn(n, D, device="cuda", generator=g)
    y = torch.randn(n, D, device="cuda", generator=g) * 1.05 + 0.05
z = torch.cat([x, y])
E = twosample.permutations(n, n, P, 0).cuda()
sigma = twosample.median_distance(z).item()
gamma = [1.0 / (2.0 * (s * sigma) ** 2) for s in (0.5, 1.0, 2.0)]


@torch.no_grad()
def torch_mmd():
    zc = z.double()
    zc = zc - zc.mean(dim=0)
    nrm = (zc * zc).sum(dim=1)
    Ef = E.t().double().contiguous()                                   # [N, P]
    acc_a = torch.zeros(P, dtype=torch.float64, device="cuda")
    row_all = torch.empty(N, dtype=torch.float64, device="cuda")
    for r0 in range(0, N, CHUNK):
        r1 = min(N, r0 + CHUNK)
        d2 = (nrm[r0:r1, None] + nrm[None, :] - 2.0 * (zc[r0:r1] @ zc.t())).clamp_min_(0.0)
        if kernel == "energy":
            K = -d2.sqrt_()
        else:
            K = torch.zeros_like(d2)
            for gq in gamma:
                K += torch.exp(-gq * d2)
            K /= len(gamma)
        K[torch.arange(r1 - r0, device="cuda"), torch.arange(r0, r1, device="cuda")] = 0.0
        acc_a += (Ef[r0:r1] * (K @ Ef)).sum(dim=0)
        row_all[r0:r1] = K.sum(dim=1)
    b, c = row_all @ Ef, row_all.sum()
    nn = Ef.sum(dim=0)
    mm = N - nn
    return acc_a / (nn * (nn - 1)) + (c - 2 * b + acc_a) / (mm * (mm - 1)) - 2 * (b - acc_a) / (nn * mm)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


fns = {"hip_mmd_test": lambda: twosample.mmd_test(x, y, n_perms=P, kernel=kernel),
       "hip_mmd": lambda: twosample.mmd(z, E, kernel, gamma),
       "hip_mmd_one_split": lambda: twosample.mmd(z, E[:1], kernel, gamma),
       "torch_mmd": torch_mmd}
for fn in fns.values():                                  # warm-up: code objects, the caching allocator, rocBLAS's choices
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in fns}
for r in range(rounds):                                  # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k]))
out = {"n": n, "m": n, "D": D, "P": P, "kernel": kernel, "rounds": rounds, "torch_chunk": CHUNK, "sigma": sigma,
       "workspace_bytes": twosample.workspace_bytes(N, D, P)}
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
out["hip_gram_part_ms"] = out["hip_mmd_one_split_ms"]
out["hip_permutation_part_ms"] = round(out["hip_mmd_ms"] - out["hip_mmd_one_split_ms"], 3)
out["torch_over_hip_mmd"] = round(out["torch_mmd_ms"] / out["hip_mmd_ms"], 3)
got, ref = twosample.mmd(z, E, kernel, gamma)[0], torch_mmd()
out["max_diff_vs_torch"] = float((got - ref).abs().max())
out["mmd2"] = float(got[0])
print(json.dumps(out), flush=True)
