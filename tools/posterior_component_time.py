"""Time of Engine.posterior_component (include/gmvae_hip.h gmvae_posterior_component: the VAE_GMP's posterior over the component of
its mixture prior by importance sampling) against Engine.iw_bound on the same vae_gmp engine, inputs, number of samples and chunk
-- the same forward per chunk, one fold per (row, component) instead of one per row -- with device events after a warm-up, in
alternating rounds:
    python tools/posterior_component_time.py [B] [n] [chunk] [rounds] [reps]
(default: the reference's default sizes, B = 1024, n = 5000, chunk 50, 7 rounds of 3 calls each).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd.engine import Engine

a = sys.argv[1:]
B, n, chunk, rounds, reps = (int(v) for v in (a[:5] + ["1024", "5000", "50", "7", "3"][len(a[:5]):]))
K = 10
x = torch.from_numpy((np.random.default_rng(0).random((B, 784)) < 0.87).astype(np.uint8)).cuda()
e = Engine("vae_gmp", 784, 64, K, [64], random_seed=0)
fns = {"posterior_component": lambda: e.posterior_component(x, n, chunk=chunk), "iw_bound": lambda: e.iw_bound(x, n, chunk=chunk)}


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


for fn in fns.values():                              # warm-up: workspaces, code objects
    fn()
torch.cuda.synchronize()
ms = {k: [] for k in fns}
for r in range(rounds):                              # alternating rounds, the order swapped every round
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        ms[k].append(timed(fns[k], reps))
o, ob = e.posterior_component(x, n, chunk=chunk), e.iw_bound(x, n, chunk=chunk)
med = {k: float(np.median(v)) for k, v in ms.items()}
nch = (n + chunk - 1) // chunk
print(json.dumps({"B": B, "n_samples": n, "K": K, "chunk": chunk, "chunks": nch, "rounds": rounds, "reps": reps,
                  "posterior_component_ms": round(med["posterior_component"], 4),
                  "posterior_component_min_max_ms": [round(min(ms["posterior_component"]), 4), round(max(ms["posterior_component"]), 4)],
                  "iw_bound_ms": round(med["iw_bound"], 4),
                  "iw_bound_min_max_ms": [round(min(ms["iw_bound"]), 4), round(max(ms["iw_bound"]), 4)],
                  "posterior_over_iw_bound": round(med["posterior_component"] / med["iw_bound"], 4),
                  "extra_ms": round(med["posterior_component"] - med["iw_bound"], 4),
                  "extra_us_per_chunk": round((med["posterior_component"] - med["iw_bound"]) * 1e3 / nch, 3),
                  "sample_rows_per_s": round(B * n / (med["posterior_component"] * 1e-3)),
                  "bound_max_rel_diff": float(((o["bound"] - ob["bound"]).abs() / ob["bound"].abs()).max().item()),
                  "mean_ess": float(o["ess"].double().mean().item()), "mean_entropy": float(o["entropy"].double().mean().item()),
                  "mean_kl_post_prior": float(o["kl_post_prior"].double().mean().item()),
                  "finite": bool(all(torch.isfinite(v).all().item() for v in o.values()))}), flush=True)
