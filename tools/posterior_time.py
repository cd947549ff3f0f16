"""Time of Engine.posterior_y (include/gmvae_hip.h gmvae_posterior_y: the posterior over y by importance sampling per component)
against Engine.iw_bound_enum_y on the same engine, inputs, number of samples and chunk -- the same forward per chunk, another
merge -- with device events after a warm-up, in alternating rounds:
    python tools/posterior_time.py [B] [n] [chunk] [rounds] [reps]
(default: the reference's default sizes, B = 1024, n = 500, chunk 5, 7 rounds of 3 calls each).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd.engine import Engine

a = sys.argv[1:]
B, n, chunk, rounds, reps = (int(v) for v in (a[:5] + ["1024", "500", "5", "7", "3"][len(a[:5]):]))
K = 10
x = torch.from_numpy((np.random.default_rng(0).random((B, 784)) < 0.87).astype(np.uint8)).cuda()
e = Engine("gmvae", 784, 64, K, [64], random_seed=0)
fns = {"posterior_y": lambda: e.posterior_y(x, n, chunk=chunk), "iw_bound_enum_y": lambda: e.iw_bound_enum_y(x, n, chunk=chunk)}


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
o, ob = e.posterior_y(x, n, chunk=chunk), e.iw_bound_enum_y(x, n, chunk=chunk)
med = {k: float(np.median(v)) for k, v in ms.items()}
nch = (n + chunk - 1) // chunk
print(json.dumps({"B": B, "n_samples": n, "K": K, "chunk": chunk, "chunks": nch, "rounds": rounds, "reps": reps,
                  "posterior_y_ms": round(med["posterior_y"], 4), "posterior_y_min_max_ms": [round(min(ms["posterior_y"]), 4),
                                                                                             round(max(ms["posterior_y"]), 4)],
                  "iw_bound_enum_y_ms": round(med["iw_bound_enum_y"], 4),
                  "iw_bound_enum_y_min_max_ms": [round(min(ms["iw_bound_enum_y"]), 4), round(max(ms["iw_bound_enum_y"]), 4)],
                  "posterior_over_enum": round(med["posterior_y"] / med["iw_bound_enum_y"], 4),
                  "extra_us_per_chunk": round((med["posterior_y"] - med["iw_bound_enum_y"]) * 1e3 / nch, 3),
                  "bound_max_rel_diff": float(((o["bound"] - ob["bound"]).abs() / ob["bound"].abs()).max().item()),
                  "mean_ess": float(o["ess"].double().mean().item()), "mean_entropy": float(o["entropy"].double().mean().item()),
                  "mean_kl_q_post": float(o["kl_q_post"].double().mean().item()),
                  "finite": bool(all(torch.isfinite(v).all().item() for v in o.values()))}), flush=True)
