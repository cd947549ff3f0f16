"""Time of the training step under the weighted objective (Engine(weighted_objective=True), include/gmvae_hip.h GMVAE_OBJ_WEIGHTS)
next to the step without the bit, configs[2] sizes: (a) the GMVAE with y summed out (y_inference="marginal") without and with the
bit -- the launches are replaced one for one, plus wobj_tail -- and (b) the Gumbel GMVAE and the VAE with the bit, which take the
general schedule, against their one-launch steps without it.
The method of tools/semisup_time.py: each configuration is a captured 16-step train graph timed with device events after a
warm-up; the configurations alternate over rounds; per configuration the median and the min - max spread over the rounds:
    python tools/wobj_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--steps 16] [--launches 4] [--rounds 21] [--only NAME]
--only NAME (marginal_plain, marginal_weights, gumbel_plain, gumbel_weights, vae_plain, vae_weights) times one configuration,
e.g. under `rocprofv3 --kernel-trace --stats` for its launch list.  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("steps", 16), ("launches", 4), ("rounds", 21)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--only", default=None)
a = ap.parse_args()
Lz, K, H, n, B = a.latent, a.K, a.hidden, a.steps, a.B

WOBJ = dict(weighted_objective=True, kl_weight=0.5, y_weight=2.0, y_free_nats=0.1)
CONFIGS = {}
for fam, model, kw in (("marginal", "gmvae", dict(y_inference="marginal")), ("gumbel", "gmvae", {}), ("vae", "vae", {})):
    CONFIGS[f"{fam}_plain"] = (model, kw)
    CONFIGS[f"{fam}_weights"] = (model, dict(kw, **WOBJ))
if a.only:
    CONFIGS = {a.only: CONFIGS[a.only]}
rng = np.random.default_rng(0)
x = torch.from_numpy((rng.random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()
warm = torch.tensor([[0.5 * min(1.0, (i + 1) / n), 2.0 * min(1.0, (i + 1) / n), 0.1, 0.0] for i in range(n)], dtype=torch.float32)
graphs = {}
for name, (model, kw) in CONFIGS.items():
    e = Engine(model, 784, Lz, K if model == "gmvae" else 1, [H], random_seed=0, **kw)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x)
    if e.weighted_objective:
        replay.obj_weights.copy_(warm)                                 # a warm-up over the graph's steps
    replay()                                                           # warm-up
    graphs[name] = (e, replay)
torch.cuda.synchronize()
times = {name: [] for name in graphs}
for _ in range(a.rounds):
    for name, (e, replay) in graphs.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            replay()
        t1.record()
        torch.cuda.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3 / (a.launches * n))
res = {"latent": Lz, "K": K, "hidden": H, "B": B, "steps_per_graph": n, "launches": a.launches, "rounds": a.rounds,
       "step_us": {}, "min_us": {}, "max_us": {}, "schedules": {}, "losses": {}}
for name, (e, replay) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["min_us"][name] = round(float(np.min(times[name])), 2)
    res["max_us"][name] = round(float(np.max(times[name])), 2)
    res["schedules"][name] = L.step_schedule(e.dims(B), e.model)
    res["losses"][name] = float((tail[0] / tail[4]).item())
    e.drop_graphs()
st = res["step_us"]
if "marginal_weights" in st and "marginal_plain" in st:
    res["marginal_weights_minus_plain_us"] = round(st["marginal_weights"] - st["marginal_plain"], 2)
    res["marginal_plain_spread_us"] = round(res["max_us"]["marginal_plain"] - res["min_us"]["marginal_plain"], 2)
for fam in ("gumbel", "vae"):
    if f"{fam}_weights" in st and f"{fam}_plain" in st:
        res[f"{fam}_weights_over_plain"] = round(st[f"{fam}_weights"] / st[f"{fam}_plain"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
