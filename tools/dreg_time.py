"""Time of the training step with the doubly reparameterised gradient (Engine(grad_estimator="dreg"), include/gmvae_hip.h
GMVAE_GRAD_DREG) next to the standard estimator on the same engine sizes: the GMVAE with y summed out at S = 5
(y_inference="marginal_iw") and the VAE_GMP at B = 256, S = 50, both at configs[2] sizes otherwise.  The method of
tools/ymarg_iw_time.py: each configuration is a captured multi-step train graph timed with device events after a warm-up; the
configurations alternate over rounds; per configuration the median and the min - max spread over the rounds:
    python tools/dreg_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--steps 16] [--launches 10] [--rounds 7]
                              [--gmp_B 256] [--gmp_S 50] [--iw_S 5] [--only NAME]
--only NAME (iw_standard, iw_dreg, gmp_standard, gmp_dreg) times one configuration, e.g. under `rocprofv3 --kernel-trace
--stats` for its launch list.  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("steps", 16), ("launches", 10), ("rounds", 7),
             ("gmp_B", 256), ("gmp_S", 50), ("iw_S", 5)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--only", default=None)
a = ap.parse_args()
Lz, K, H, n = a.latent, a.K, a.hidden, a.steps

CONFIGS = {}
for est in L.GRAD_ESTIMATORS:
    CONFIGS[f"iw_{est}"] = ("gmvae", a.B, dict(y_inference="marginal_iw", n_samples=a.iw_S, grad_estimator=est))
    CONFIGS[f"gmp_{est}"] = ("vae_gmp", a.gmp_B, dict(n_samples=a.gmp_S, grad_estimator=est))
if a.only:
    CONFIGS = {a.only: CONFIGS[a.only]}
graphs = {}
for name, (model, B, kw) in CONFIGS.items():
    x = torch.from_numpy((np.random.default_rng(0).random((n, B, 784)) < 0.87).astype(np.uint8)).cuda()
    e = Engine(model, 784, Lz, K, [H], random_seed=0, **kw)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x)
    replay()                                                           # warm-up
    graphs[name] = (e, replay, B)
torch.cuda.synchronize()
times = {name: [] for name in graphs}
for _ in range(a.rounds):
    for name, (e, replay, B) in graphs.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            replay()
        t1.record()
        torch.cuda.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3 / (a.launches * n))
res = {"latent": Lz, "K": K, "hidden": H, "steps_per_graph": n, "launches": a.launches, "rounds": a.rounds, "step_us": {},
       "min_us": {}, "max_us": {}, "rows": {}, "schedules": {}, "losses": {}}
for name, (e, replay, B) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["min_us"][name] = round(float(np.min(times[name])), 2)
    res["max_us"][name] = round(float(np.max(times[name])), 2)
    res["rows"][name] = B * e.rows_per_x
    res["schedules"][name] = L.step_schedule(e.dims(B), e.model)
    res["losses"][name] = float((tail[0] / tail[4]).item())
    e.drop_graphs()
st = res["step_us"]
for fam in ("iw", "gmp"):
    if f"{fam}_dreg" in st and f"{fam}_standard" in st:
        res[f"{fam}_dreg_minus_standard_us"] = round(st[f"{fam}_dreg"] - st[f"{fam}_standard"], 2)
        res[f"{fam}_standard_spread_us"] = round(res["max_us"][f"{fam}_standard"] - res["min_us"][f"{fam}_standard"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
