"""us/step of the training step at the configs[2] sizes (GMVAE, B = 1024, D = 784, H = 64, L = 64, K = 10) inside a 32-step train
graph, HIP events around each graph launch, warm clocks, median of the repeats -- with and without gradient clipping
(profiles/clip_notes.md).  The schedule is whatever the GMVAE_NO_* switches of the environment leave (GMVAE_NO_MEGA=1
GMVAE_NO_SKINNY=1 GMVAE_NO_FUSED=1: the general schedule).
argv: [--clip_norm C] [--tree DIR (another checkout of the project, built; default: this one)] [--seconds S]"""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--clip_norm", type=float, default=None)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--seconds", type=float, default=2.0)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine
G, B, D = 32, 1024, 784
kw = {} if a.clip_norm is None else dict(clip_norm=a.clip_norm)
e = Engine("gmvae", D, 64, 10, [64], random_seed=0, **kw)
sx, replay = e.capture_train_step(B, 1e-3, n_steps=G)
sx.copy_(torch.from_numpy((np.random.default_rng(0).random((G, B, D)) < 0.87).astype(np.uint8)).cuda())
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.7:
    replay()
torch.cuda.synchronize()
ms = []
t0 = time.perf_counter()
while time.perf_counter() - t0 < a.seconds:
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for s, f in evs:
        s.record(); replay(); f.record()
    torch.cuda.synchronize()
    ms += [s.elapsed_time(f) / G for s, f in evs]
ms.sort()
out = {"schedule": L.step_schedule(e.dims(B), e.model), "clip_norm": a.clip_norm, "us_per_step_median": round(ms[len(ms) // 2] * 1e3, 2),
       "us_per_step_min": round(ms[0] * 1e3, 2), "launches": len(ms), "loss": e.grads[e.P].item() / B,
       "levels": [n for n, _, _ in e.profile_levels(sx[0], iters=2)]}
if a.clip_norm is not None:
    r = replay.grad_clip.cpu()
    out["clipped_share"], out["grad_norm_last"] = float(r[:, 2].mean()), float(r[-1, 0])
print(json.dumps(out))
