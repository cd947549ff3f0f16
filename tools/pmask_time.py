"""Time of the training step under a per-example observation mask (Engine(pixel_mask=True), include/gmvae_hip.h
GMVAE_OBJ_PIXEL_MASK) next to general-schedule steps without the bit, configs[2] sizes: the one-launch step, the general schedule
without any bit (the library's GMVAE_NO_MEGA / GMVAE_NO_SKINNY / GMVAE_NO_FUSED switches during its capture), the weighted
objective at weights (1, 1, 0) -- a general-schedule step the parent commit has too -- and general+mask with a mask of rate 0.3 per
step.
The method of tools/ytemp_time.py: each configuration is a captured 16-step train graph timed with device events after a
warm-up; the configurations alternate over rounds; per configuration the median and the min - max spread over the rounds:
    python tools/pmask_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--S 1] [--steps 16] [--launches 4] [--rounds 21]
Prints one JSON line.
    python tools/pmask_time.py --eager-steps N
runs N eager masked training steps after a warm-up and nothing else: the program of a kernel trace (rocprofv3 --kernel-trace
--stats -- python tools/pmask_time.py --eager-steps 200), whose per-kernel totals give each launch's share of the step."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("S", 1), ("steps", 16), ("launches", 4), ("rounds", 21),
             ("eager-steps", 0)):
    ap.add_argument(f"--{k}", type=int, default=v)
a = ap.parse_args()
Lz, K, H, n, B, S = a.latent, a.K, a.hidden, a.steps, a.B, a.S

rng = np.random.default_rng(0)
x = torch.from_numpy((rng.random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()
masks = torch.from_numpy((rng.random((n, B, 784)) >= 0.3).astype(np.uint8)).cuda()

if a.eager_steps > 0:
    e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, pixel_mask=True)
    for i in range(8):                                                     # warm-up: code objects, the workspace
        e.train_step(x[i % n], lr=1e-3, mask=masks[i % n])
    torch.cuda.synchronize()
    for i in range(a.eager_steps):
        e.train_step(x[i % n], lr=1e-3, mask=masks[i % n])
    torch.cuda.synchronize()
    tail = e.grads[e.P:].double()
    print(json.dumps({"eager_steps": a.eager_steps, "schedule": L.step_schedule(e.dims(B), e.model),
                      "loss": float((tail[0] / tail[4]).item()), "observed_share": float((tail[7] / (tail[6] + tail[7])).item())}))
    sys.exit(0)

GENERAL = {"GMVAE_NO_MEGA": "1", "GMVAE_NO_SKINNY": "1", "GMVAE_NO_FUSED": "1"}
CONFIGS = {"one_launch": ({}, {}), "general": ({}, GENERAL), "general_weights": (dict(weighted_objective=True), {}),
           "general_mask": (dict(pixel_mask=True), {})}
if S != 1:
    del CONFIGS["general_weights"]                                         # (the weighted objective is the one-sample bound's)


def capture(kw, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, **kw)
        sched = L.step_schedule(e.dims(B), e.model)
        sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
        sx.copy_(x)
        if e.pixel_mask:
            replay.pixel_mask.copy_(masks)                                 # one mask per step of the graph
        replay()                                                           # warm-up
        torch.cuda.synchronize()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return e, replay, sched


graphs = {name: capture(kw, env) for name, (kw, env) in CONFIGS.items()}
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
res["mask_minus_general_us"] = round(st["general_mask"] - st["general"], 2)
res["general_spread_us"] = round(res["max_us"]["general"] - res["min_us"]["general"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
for name, (e, _, _) in graphs.items():
    e.drop_graphs()
