"""Time of the training step under a likelihood on grey-level bytes (Engine(likelihood=), include/gmvae_hip.h GMVAE_LIK_*) next
to the masked step at an all-ones mask -- the same GEMMs on the same general schedule with an epilogue of comparable weight --,
configs[2] sizes: general+mask, general+grey, general+cb, general+gauss (sigma 0.25).
The method of tools/pmask_time.py: each configuration is a captured 16-step train graph timed with device events after a
warm-up; the configurations alternate over rounds; per configuration the median and the min - max spread over the rounds:
    python tools/lik_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--S 1] [--steps 16] [--launches 4] [--rounds 21]
Prints one JSON line.
    python tools/lik_time.py --eager-steps N [--likelihood continuous_bernoulli]
runs N eager training steps under that likelihood after a warm-up and nothing else: the program of a kernel trace (rocprofv3
--kernel-trace --stats -- python tools/lik_time.py --eager-steps 200), whose per-kernel totals give each launch's share of the
step; --likelihood mask runs the masked step at an all-ones mask instead."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("S", 1), ("steps", 16), ("launches", 4), ("rounds", 21),
             ("eager-steps", 0)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--likelihood", default="continuous_bernoulli", choices=list(L.LIKELIHOODS)[1:] + ["mask"])
a = ap.parse_args()
Lz, K, H, n, B, S = a.latent, a.K, a.hidden, a.steps, a.B, a.S

rng = np.random.default_rng(0)
grey = rng.integers(0, 256, size=(n, B, 784))
r = rng.random((n, B, 784))
grey[r < 0.3] = 0
grey[r >= 0.9] = 255
x = torch.from_numpy(grey.astype(np.uint8)).cuda()
x01 = (x >= 128).to(torch.uint8)                                           # (the masked step's batch: bytes in {0, 1})

CONFIGS = {"general_mask": dict(pixel_mask=True), "general_grey": dict(likelihood="grey_bernoulli"),
           "general_cb": dict(likelihood="continuous_bernoulli"), "general_gauss": dict(likelihood="gaussian", likelihood_sigma=0.25)}

if a.eager_steps > 0:
    kw = dict(pixel_mask=True) if a.likelihood == "mask" else dict(likelihood=a.likelihood, likelihood_sigma=0.25)
    e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, **kw)
    xs = x01 if a.likelihood == "mask" else x
    for i in range(8):                                                     # warm-up: code objects, the workspace
        e.train_step(xs[i % n], lr=1e-3)
    torch.cuda.synchronize()
    for i in range(a.eager_steps):
        e.train_step(xs[i % n], lr=1e-3)
    torch.cuda.synchronize()
    tail = e.grads[e.P:].double()
    print(json.dumps({"eager_steps": a.eager_steps, "schedule": L.step_schedule(e.dims(B), e.model),
                      "loss": float((tail[0] / tail[4]).item()), "tail5_over_tail6": float((tail[5] / tail[6]).item())}))
    sys.exit(0)


def capture(kw):
    e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, **kw)
    sched = L.step_schedule(e.dims(B), e.model)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x01 if e.pixel_mask else x)                                   # (the masks stay as pre-filled: all observed)
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
       "step_us": {}, "min_us": {}, "max_us": {}, "schedules": {}, "losses": {}, "recon_mse": {}}
for name, (e, replay, sched) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["min_us"][name] = round(float(np.min(times[name])), 2)
    res["max_us"][name] = round(float(np.max(times[name])), 2)
    res["schedules"][name] = sched
    res["losses"][name] = float((tail[0] / tail[4]).item())
    if not e.pixel_mask:
        res["recon_mse"][name] = float((tail[5] / tail[6]).item())
st = res["step_us"]
for name in ("general_grey", "general_cb", "general_gauss"):
    res[f"{name}_minus_mask_us"] = round(st[name] - st["general_mask"], 2)
res["mask_spread_us"] = round(res["max_us"]["general_mask"] - res["min_us"]["general_mask"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
for name, (e, _, _) in graphs.items():
    e.drop_graphs()
