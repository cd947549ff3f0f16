"""Time of the training step on real-valued rows (Engine(real_valued=True), include/gmvae_hip.h GMVAE_X_F32) next to the
grey-level Gaussian step it skips the t pass of, and what the learned scale's rho reduction (GMVAE_LIK_SCALE_LEARNED,
csrc/liksig.hpp) adds -- configs[2] sizes (GMVAE 784-64-64-10, B = 1024): general+gauss on bytes, general+gauss+f32 on the same
values as floats (bytes / 255), general+gauss+f32+lsig.
The method of tools/lik_time.py: each configuration is a captured 16-step train graph timed with device events after a warm-up;
the configurations alternate over the rounds in one process; per configuration the median and the min - max spread:
    python tools/realx_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--S 1] [--steps 16] [--launches 4] [--rounds 21]
Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("S", 1), ("steps", 16), ("launches", 4), ("rounds", 21)):
    ap.add_argument(f"--{k}", type=int, default=v)
a = ap.parse_args()
Lz, K, H, n, B, S = a.latent, a.K, a.hidden, a.steps, a.B, a.S

rng = np.random.default_rng(0)
grey = rng.integers(0, 256, size=(n, B, 784))
r = rng.random((n, B, 784))
grey[r < 0.3] = 0
grey[r >= 0.9] = 255
xb = torch.from_numpy(grey.astype(np.uint8)).cuda()
xf = torch.from_numpy(grey.astype(np.float32) / np.float32(255)).cuda()      # (the same t, as floats)

GA = dict(likelihood="gaussian", likelihood_sigma=0.25)
CONFIGS = {"gauss_bytes": GA, "gauss_f32": dict(real_valued=True, **GA),
           "gauss_f32_lsig": dict(real_valued=True, likelihood_scale="learned", **GA)}


def capture(kw):
    e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, **kw)
    sched = L.step_schedule(e.dims(B), e.model)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(xf if e.real_valued else xb)
    replay()                                                               # warm-up
    torch.cuda.synchronize()
    return e, replay, sched


graphs = {name: capture(kw) for name, kw in CONFIGS.items()}
torch.cuda.synchronize()
times = {name: [] for name in graphs}
for _ in range(a.rounds):
    for name, (e, replay, _) in graphs.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            replay()
        t1.record()
        torch.cuda.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3 / (a.launches * n))
res = {"latent": Lz, "K": K, "hidden": H, "B": B, "S": S, "steps_per_graph": n, "launches": a.launches, "rounds": a.rounds,
       "step_us": {}, "min_us": {}, "max_us": {}, "schedules": {}, "losses": {}}
for name, (e, replay, sched) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["min_us"][name] = round(float(np.min(times[name])), 2)
    res["max_us"][name] = round(float(np.max(times[name])), 2)
    res["schedules"][name] = sched
    res["losses"][name] = float((tail[0] / tail[4]).item())
st = res["step_us"]
res["f32_minus_bytes_us"] = round(st["gauss_f32"] - st["gauss_bytes"], 2)
res["lsig_minus_f32_us"] = round(st["gauss_f32_lsig"] - st["gauss_f32"], 2)
res["bytes_spread_us"] = round(res["max_us"]["gauss_bytes"] - res["min_us"]["gauss_bytes"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
for name, (e, _, _) in graphs.items():
    e.drop_graphs()
