"""Time of the Gumbel GMVAE's training step with the temperature on the device (Engine(temperature_on_device=True),
include/gmvae_hip.h GMVAE_Y_TEMP_DEV) and under the straight-through y (y_estimator="straight_through", GMVAE_Y_STRAIGHT_THROUGH)
next to the step without the bits, configs[2] sizes: the one-launch step, the general schedule without the bits (the library's
GMVAE_NO_MEGA / GMVAE_NO_SKINNY / GMVAE_NO_FUSED switches during its capture), general+temp and general+temp+st.
--other-lib PATH adds the one-launch step of ANOTHER BUILD of the same ABI (the parent commit's libgmvae_hip.so) to the same
session, interleaved with the rest.
The method of tools/wobj_time.py: each configuration is a captured 16-step train graph timed with device events after a
warm-up; the configurations alternate over rounds; per configuration the median and the min - max spread over the rounds:
    python tools/ytemp_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--S 1] [--steps 16] [--launches 4] [--rounds 21]
                               [--other-lib PATH]
Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("S", 1), ("steps", 16), ("launches", 4), ("rounds", 21)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--other-lib", default=None)
a = ap.parse_args()
Lz, K, H, n, B, S = a.latent, a.K, a.hidden, a.steps, a.B, a.S

GENERAL = {"GMVAE_NO_MEGA": "1", "GMVAE_NO_SKINNY": "1", "GMVAE_NO_FUSED": "1"}
CONFIGS = {"one_launch": ({}, {}), "general": ({}, GENERAL), "general_temp": (dict(temperature_on_device=True), {}),
           "general_temp_st": (dict(temperature_on_device=True, y_estimator="straight_through"), {})}
rng = np.random.default_rng(0)
x = torch.from_numpy((rng.random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()
anneal = torch.tensor([max(0.5, 2.0 * np.exp(-0.05 * i)) for i in range(n)], dtype=torch.float32)


def capture(kw, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, **kw)
        sched = L.step_schedule(e.dims(B), e.model)
        sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
        sx.copy_(x)
        if e.temperature_on_device:
            replay.y_temperature.copy_(anneal)                             # an annealing over the graph's steps
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
own, own_path, other = L.lib, L.LIB_PATH, None
if a.other_lib:                                    # the other build's one-launch step: its graph is created and launched by ITS library
    L.LIB_PATH = os.path.abspath(a.other_lib)
    other, _ = L._load()
    L.lib = other
    try:
        graphs["other_one_launch"] = capture({}, {})
    finally:
        L.lib, L.LIB_PATH = own, own_path
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
res["temp_minus_general_us"] = round(st["general_temp"] - st["general"], 2)
res["st_minus_temp_us"] = round(st["general_temp_st"] - st["general_temp"], 2)
res["general_spread_us"] = round(res["max_us"]["general"] - res["min_us"]["general"], 2)
if "other_one_launch" in st:
    res["one_launch_over_other"] = round(st["one_launch"] / st["other_one_launch"], 4)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
for name, (e, _, _) in graphs.items():              # (the other build's graph handles are destroyed by its library)
    if name == "other_one_launch":
        L.lib = other
    e.drop_graphs()
    L.lib = own
