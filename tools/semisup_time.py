"""Time of the semi-supervised training step (Engine(semi_supervised=True), include/gmvae_hip.h GMVAE_OBJ_LABELS) next to the step
without the bit on the same engine sizes: the GMVAE with y summed out at S = 1 (y_inference="marginal") and at S = 5
("marginal_iw"), configs[2] sizes otherwise, (a) without the bit and (b) with the bit and --labelled of the examples labelled.
The method of tools/dreg_time.py: each configuration is a captured 16-step train graph timed with device events after a warm-up;
the configurations alternate over rounds (A/B/A/B); per configuration the median and the min - max spread over the rounds:
    python tools/semisup_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--steps 16] [--launches 4] [--rounds 21]
                                 [--iw_S 5] [--labelled 0.1] [--only NAME]
--only NAME (marginal_plain, marginal_labels, iw_plain, iw_labels) times one configuration, e.g. under `rocprofv3 --kernel-trace
--stats` for its launch list.  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("steps", 16), ("launches", 4), ("rounds", 21), ("iw_S", 5)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--labelled", type=float, default=0.1)
ap.add_argument("--only", default=None)
a = ap.parse_args()
Lz, K, H, n, B = a.latent, a.K, a.hidden, a.steps, a.B

CONFIGS = {}
for fam, kw in (("marginal", dict(y_inference="marginal")), ("iw", dict(y_inference="marginal_iw", n_samples=a.iw_S))):
    CONFIGS[f"{fam}_plain"] = kw
    CONFIGS[f"{fam}_labels"] = dict(kw, semi_supervised=True, sup_weight=1.0)
if a.only:
    CONFIGS = {a.only: CONFIGS[a.only]}
rng = np.random.default_rng(0)
x = torch.from_numpy((rng.random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()
y = torch.from_numpy(np.where(rng.random((n, B)) < a.labelled, rng.integers(0, K, (n, B)), -1).astype(np.int32)).cuda()
graphs = {}
for name, kw in CONFIGS.items():
    e = Engine("gmvae", 784, Lz, K, [H], random_seed=0, **kw)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x)
    if e.semi_supervised:
        replay.y_observed.copy_(y)
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
       "labelled_share": a.labelled, "step_us": {}, "min_us": {}, "max_us": {}, "schedules": {}, "losses": {}, "labelled": {}}
for name, (e, replay) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["min_us"][name] = round(float(np.min(times[name])), 2)
    res["max_us"][name] = round(float(np.max(times[name])), 2)
    res["schedules"][name] = L.step_schedule(e.dims(B), e.model)
    res["losses"][name] = float((tail[0] / tail[4]).item())
    res["labelled"][name] = float(tail[6].item())
    e.drop_graphs()
st = res["step_us"]
for fam in ("marginal", "iw"):
    if f"{fam}_labels" in st and f"{fam}_plain" in st:
        res[f"{fam}_labels_minus_plain_us"] = round(st[f"{fam}_labels"] - st[f"{fam}_plain"], 2)
        res[f"{fam}_plain_spread_us"] = round(res["max_us"][f"{fam}_plain"] - res["min_us"][f"{fam}_plain"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
