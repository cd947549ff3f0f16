"""Time of the GMVAE training step with y summed out over its K components (Engine(y_inference="marginal"), include/gmvae_hip.h
GMVAE_OBJ_MARGINAL_Y) next to the Gumbel step at S = K -- the same R = B*K rows -- and the S = 1 headline step, each as a
captured multi-step train graph timed with device events after a warm-up:
    python tools/ymarg_time.py [latent] [K] [B] [hidden] [steps per graph] [launches]
(default: configs[2] -- latent 64, K 10, B 1024, hidden 64 -- 16 steps per graph, 20 launches).  Prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

a = sys.argv[1:]
Lz, K, B, H, n, reps = (int(v) for v in (a[:6] + ["64", "10", "1024", "64", "16", "20"][len(a[:6]):]))
x = torch.from_numpy((np.random.default_rng(0).random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()


def step_us(**kw):
    e = Engine("gmvae", 784, Lz, K, [H], random_seed=0, **kw)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x)
    replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        replay()
    t1.record()
    torch.cuda.synchronize()
    tail = replay.tail_log[-1].double()
    sched = L.step_schedule(e.dims(B), e.model)
    out = (t0.elapsed_time(t1) * 1e3 / (reps * n), float((tail[0] / tail[4]).item()), sched)
    e.drop_graphs()
    return out


mg = step_us(y_inference="marginal")
gk = step_us(n_samples=K)
g1 = step_us()
print(json.dumps({"latent": Lz, "K": K, "B": B, "hidden": H, "rows": B * K, "steps_per_graph": n,
                  "marginal_step_us": round(mg[0], 2), "gumbel_S_K_step_us": round(gk[0], 2), "gumbel_S1_step_us": round(g1[0], 2),
                  "marginal_over_gumbel_S_K": round(mg[0] / gk[0], 3),
                  "schedules": {"marginal": mg[2], "gumbel_S_K": gk[2], "gumbel_S1": g1[2]},
                  "losses": {"marginal": mg[1], "gumbel_S_K": gk[1], "gumbel_S1": g1[1]},
                  "finite": all(np.isfinite([mg[1], gk[1], g1[1]]))}), flush=True)
