"""Time of Engine.iw_bound (include/gmvae_hip.h gmvae_iw_bound) against the one-shot eval_iwae pass it streams, with CUDA events
after a warm-up:   python tools/iw_bound_time.py [model] [latent] [K] [B] [n] [chunk]
(default: gmvae, the reference's default sizes, B = 1024, n = 5000, chunk = 50).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd.engine import Engine

a = sys.argv[1:]
model = a[0] if len(a) > 0 else "gmvae"
Lz, K, B, n, chunk = (int(v) for v in (a[1:6] + ["64", "10", "1024", "5000", "50"][len(a[1:6]):]))
x = torch.from_numpy((np.random.default_rng(0).random((B, 784)) < 0.87).astype(np.uint8)).cuda()
e = Engine(model, 784, Lz, K, [64], n_samples=chunk, random_seed=0)


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


iw_ms = timed(lambda: e.iw_bound(x, n, chunk=chunk), 10)
fw_ms = timed(lambda: e.forward(x, n_samples=chunk), 50)        # the eval_iwae pass (B x chunk rows, images reused)
o = e.iw_bound(x, n, chunk=chunk)
print(json.dumps({"model": model, "latent": Lz, "K": K, "B": B, "n_samples": n, "chunk": chunk,
                  "iw_bound_ms": round(iw_ms, 4), "sample_rows_per_s": round(B * n / (iw_ms * 1e-3)),
                  "one_chunk_forward_us": round(fw_ms * 1e3, 2), "iw_over_forward": round(iw_ms / fw_ms, 2),
                  "chunks": (n + chunk - 1) // chunk, "mean_bound": float(o["bound"].double().mean().item()),
                  "finite": bool(torch.isfinite(o["bound"]).all().item())}), flush=True)
