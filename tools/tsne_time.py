"""Time of gmvae_amd.tsne (include/gmvae_hip.h gmvae_tsne_*: exact t-SNE on the device) at N codes of L dimensions -- the affinity
stage, one iteration (from a run of `iters` iterations) and the whole embed() call -- against a chunked torch implementation of
the same statement on the same device: difference-form distances in [256, N, L] blocks, the same bracket-and-bisect search on
the stored rows of a chunk (a fixed number of steps, rows that have met |H - ln perp| <= 1e-5 frozen: no host synchronisation
inside, as on the HIP path; the line reports the worst |H - ln perp| it ends with), and per iteration P rebuilt from d2 block
by block (memory O(chunk * N), as the HIP path).  The torch iteration is timed over `torch_iters` iterations.  Device events after a warm-up, alternating rounds:
    python tools/tsne_time.py [N] [L] [rounds] [iters] [torch_iters]
(default N = 10,000, L = 64, 3 rounds, 300 iterations, 10 torch iterations).  Prints one JSON line."""
import json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import tsne

a = sys.argv[1:]
N, Lz, rounds, iters, titers = (int(v) for v in (a[:5] + ["10000", "64", "3", "300", "10"][len(a[:5]):]))
PERP, BLK = 40.0, 256
SEARCH_STEPS = 40      # of the torch search: enough to bracket from beta = 1 and bisect to |H - ln perp| <= 1e-5 at these codes
rng = np.random.default_rng(0)
centers = rng.normal(0, 3, (10, Lz))
codes = torch.from_numpy((centers[np.arange(N) % 10] + rng.normal(0, 1, (N, Lz))).astype(np.float32)).cuda()
y0 = torch.from_numpy((1e-4 * rng.normal(0, 1, (N, 2))).astype(np.float32)).cuda()


@torch.no_grad()
def torch_d2(c, r0, r1):
    return (c[r0:r1, None, :] - c[None, :, :]).square().sum(dim=2)


@torch.no_grad()
def torch_affinities(c, perp):
    n = c.shape[0]
    beta, logz = torch.empty(n, device=c.device), torch.empty(n, device=c.device)
    worst = torch.zeros((), device=c.device, dtype=torch.float64)
    target = math.log(perp)
    for r0 in range(0, n, BLK):
        d2 = torch_d2(c, r0, min(r0 + BLK, n))
        rows = torch.arange(d2.shape[0], device=c.device)
        d2[rows, r0 + rows] = math.inf
        dmin = d2.min(dim=1, keepdim=True).values
        b = torch.ones(d2.shape[0], 1, device=c.device)
        lo, hi = torch.zeros_like(b), torch.full_like(b, math.inf)
        for _ in range(SEARCH_STEPS):                    # a fixed count: no host synchronisation inside, as on the HIP path
            x = -b * (d2 - dmin)
            e = x.exp()
            S = e.double().sum(dim=1, keepdim=True)
            H = S.log() - (torch.nan_to_num(x * e, nan=0.0)).double().sum(dim=1, keepdim=True) / S
            diff = H - target
            done = diff.abs() <= 1e-5
            up = (diff > 0) & ~done
            dn = (diff <= 0) & ~done
            lo, hi = torch.where(up, b, lo), torch.where(dn, b, hi)
            nb = torch.where(up, torch.where(hi.isinf(), b * 2, (b + hi) / 2), torch.where(lo == 0, b / 2, (lo + b) / 2))
            b = torch.where(done, b, nb)
        beta[r0:r0 + BLK] = b[:, 0]
        logz[r0:r0 + BLK] = (S.log() - (b * dmin).double())[:, 0].float()
        worst = torch.maximum(worst, diff.abs().max())
    return beta, logz, worst


@torch.no_grad()
def torch_iteration(c, beta, logz, y, vel, gains, alpha, momentum, lr):
    n = c.shape[0]
    attr, rep = torch.zeros(n, 2, device=c.device, dtype=torch.float64), torch.zeros(n, 2, device=c.device, dtype=torch.float64)
    Z, spl = torch.zeros((), device=c.device, dtype=torch.float64), torch.zeros((), device=c.device, dtype=torch.float64)
    for r0 in range(0, n, BLK):
        r1 = min(r0 + BLK, n)
        d2 = torch_d2(c, r0, r1)
        p = ((-beta[r0:r1, None] * d2 - logz[r0:r1, None]).exp() + (-beta[None, :] * d2 - logz[None, :]).exp()) / (2 * n)
        dy = y[r0:r1, None, :] - y[None, :, :]
        t = dy.square().sum(dim=2)
        w = 1 / (1 + t)
        rows = torch.arange(r1 - r0, device=c.device)
        p[rows, r0 + rows] = 0
        w[rows, r0 + rows] = 0
        attr[r0:r1] = ((p * w)[:, :, None] * dy).sum(dim=1)
        rep[r0:r1] = ((w * w)[:, :, None] * dy).sum(dim=1)
        Z += w.double().sum()
        spl -= (p * torch.log1p(t)).double().sum()
    grad = (4 * (alpha * attr - rep / Z)).float()
    inc = vel * grad < 0
    gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01)
    vel = momentum * vel - lr * gains * grad
    return y + vel, vel, gains, spl, Z


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


lr = max(N / 48.0, 50.0)
beta, logz, _ = tsne.affinities(codes, PERP)


def torch_iters():
    y, vel, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
    for _ in range(titers):
        y, vel, gains, _, _ = torch_iteration(codes, beta, logz, y, vel, gains, 12.0, 0.5, lr)
    return y


fns = {"hip_affinities": lambda: tsne.affinities(codes, PERP),
       "hip_embed": lambda: tsne.embed(codes, perplexity=PERP, n_iter=iters, init=y0),
       "hip_embed_0_iters": lambda: tsne.embed(codes, perplexity=PERP, n_iter=0, init=y0)}
if titers > 0:
    fns["torch_affinities"] = lambda: torch_affinities(codes, PERP)
    fns["torch_iterations"] = torch_iters
for fn in fns.values():                                  # warm-up: code objects, the caching allocator
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in fns}
for r in range(rounds):                                  # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k]))
out = {"N": N, "L": Lz, "perplexity": PERP, "rounds": rounds, "iters": iters, "torch_iters": titers, "torch_block": BLK,
       "rows_per_affinity_chunk": tsne.default_rows(N), "workspace_bytes": tsne.workspace_bytes(N, Lz, tsne.default_rows(N))}
for k, v in ms.items():
    out[f"{k}_ms"] = round(float(np.median(v)), 3)
    out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
# embed() = affinities + iters iterations + one closing gradient pass: the iteration's share by difference
out["hip_iteration_ms"] = round((out["hip_embed_ms"] - out["hip_embed_0_iters_ms"]) / max(iters, 1), 4)
out["pairs_per_s"] = round(N * (N - 1) / (out["hip_iteration_ms"] * 1e-3)) if out["hip_iteration_ms"] > 0 else None
o = tsne.embed(codes, perplexity=PERP, n_iter=iters, init=y0)
out.update(kl=float(o["kl"]), kl_first=float(o["kl_history"][0]) if iters else None, finite=bool(torch.isfinite(o["embedding"]).all()))
if titers > 0:
    out["torch_iteration_ms"] = round(out["torch_iterations_ms"] / titers, 3)
    out["torch_over_hip_iteration"] = round(out["torch_iteration_ms"] / out["hip_iteration_ms"], 1)
    out["torch_over_hip_affinities"] = round(out["torch_affinities_ms"] / out["hip_affinities_ms"], 1)
    tb, tl, tw = torch_affinities(codes, PERP)
    out["torch_search_steps"], out["torch_search_worst_entropy_error"] = SEARCH_STEPS, float(tw)
    yt = torch_iters()
    yh = tsne.embed(codes, perplexity=PERP, n_iter=titers, exaggeration_iters=titers, init=y0)["embedding"]
    out["max_rel_diff_vs_torch"] = {"beta": float(((tb - beta) / beta).abs().max()), "logz": float((tl - logz).abs().max()),
                                    "embedding": float((yt - yh).abs().max() / yh.abs().max())}
print(json.dumps(out), flush=True)
