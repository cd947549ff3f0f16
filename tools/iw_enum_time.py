"""Time of Engine.iw_bound_enum_y (include/gmvae_hip.h gmvae_iw_bound_enum_y: y summed out over K) against the Gumbel
Engine.iw_bound on the general schedule (GMVAE_NO_EVALF=1) at the same number of sample rows (n K samples), with device events
after a warm-up:   python tools/iw_enum_time.py [B] [n] [reps]
(default: the reference's default sizes, B = 1024, n = 500, the default chunks).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd.engine import Engine

a = sys.argv[1:]
B, n, reps = (int(v) for v in (a[:3] + ["1024", "500", "5"][len(a[:3]):]))
K = 10
x = torch.from_numpy((np.random.default_rng(0).random((B, 784)) < 0.87).astype(np.uint8)).cuda()
e = Engine("gmvae", 784, 64, K, [64], random_seed=0)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


enum_ms = timed(lambda: e.iw_bound_enum_y(x, n), reps)
o = e.iw_bound_enum_y(x, n)
os.environ["GMVAE_NO_EVALF"] = "1"                 # the Gumbel bound on the general schedule, like the enumerated one
gum_ms = timed(lambda: e.iw_bound(x, n * K), reps)
rows = B * n * K
print(json.dumps({"B": B, "n_samples": n, "K": K, "sample_rows": rows,
                  "enum_chunk": max(1, min(n, Engine.IW_CHUNK_ROWS // (B * K))),
                  "gumbel_chunk": max(1, min(n * K, Engine.IW_CHUNK_ROWS // B)),
                  "iw_bound_enum_y_ms": round(enum_ms, 4), "enum_sample_rows_per_s": round(rows / (enum_ms * 1e-3)),
                  "gumbel_iw_bound_no_evalf_ms": round(gum_ms, 4), "gumbel_sample_rows_per_s": round(rows / (gum_ms * 1e-3)),
                  "enum_over_gumbel": round(enum_ms / gum_ms, 3),
                  "mean_bound": float(o["bound"].double().mean().item()),
                  "mean_minus_mlw": float((o["bound"] - o["mean_logw"]).double().mean().item()),
                  "finite": bool(torch.isfinite(o["bound"]).all().item())}), flush=True)
