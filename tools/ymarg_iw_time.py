"""Time of the GMVAE training step with y summed out and z importance-weighted over S samples per component
(Engine(y_inference="marginal_iw"), include/gmvae_hip.h GMVAE_OBJ_MARGINAL_Y_IW) at S = 1, 2 and 5, next to the
single-sample marginal step (GMVAE_OBJ_MARGINAL_Y) and the Gumbel IWAE step at S*K samples -- the same R = B*S*K rows.  Each
is a captured multi-step train graph timed with device events after a warm-up; the configurations alternate over rounds and
each reports its median:
    python tools/ymarg_iw_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--steps 16] [--launches 10] [--rounds 3]
                                  [--only NAME]
(default: configs[2] sizes).  --only NAME (iw1, iw2, iw5, marginal, gumbel20, gumbel50) times one configuration, e.g. under
`rocprofv3 --kernel-trace --stats` for its launch list.  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("steps", 16), ("launches", 10), ("rounds", 3)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--only", default=None)
a = ap.parse_args()
Lz, K, B, H, n = a.latent, a.K, a.B, a.hidden, a.steps
x = torch.from_numpy((np.random.default_rng(0).random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()

CONFIGS = {"iw1": dict(y_inference="marginal_iw", n_samples=1), "iw2": dict(y_inference="marginal_iw", n_samples=2),
           "iw5": dict(y_inference="marginal_iw", n_samples=5), "marginal": dict(y_inference="marginal"),
           f"gumbel{2 * K}": dict(n_samples=2 * K), f"gumbel{5 * K}": dict(n_samples=5 * K)}
if a.only:
    CONFIGS = {a.only: CONFIGS[a.only]}
graphs = {}
for name, kw in CONFIGS.items():
    e = Engine("gmvae", 784, Lz, K, [H], random_seed=0, **kw)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x)
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
res = {"latent": Lz, "K": K, "B": B, "hidden": H, "steps_per_graph": n, "launches": a.launches, "rounds": a.rounds,
       "step_us": {}, "rows": {}, "schedules": {}, "losses": {}}
for name, (e, replay) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["rows"][name] = B * e.rows_per_x
    res["schedules"][name] = L.step_schedule(e.dims(B), e.model)
    res["losses"][name] = float((tail[0] / tail[4]).item())
    e.drop_graphs()
st = res["step_us"]
if "iw5" in st and f"gumbel{5 * K}" in st:
    res["iw5_over_gumbel"] = round(st["iw5"] / st[f"gumbel{5 * K}"], 3)
if "iw2" in st and f"gumbel{2 * K}" in st:
    res["iw2_over_gumbel"] = round(st["iw2"] / st[f"gumbel{2 * K}"], 3)
if "iw1" in st and "marginal" in st:
    res["iw1_over_marginal"] = round(st["iw1"] / st["marginal"], 3)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
