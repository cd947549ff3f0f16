"""Time of the training step on count data (Engine(likelihood="poisson" | "negative_binomial"), include/gmvae_hip.h
GMVAE_LIK_POISSON / GMVAE_LIK_NEG_BINOMIAL) next to the general-schedule steps it stands beside -- configs[2] sizes (GMVAE
784-64-64-10, B = 1024): the Bernoulli step on the general schedule (clip_norm = inf: "general+clip"), general+gauss on bytes,
general+gauss+f32+lsig, general+pois+f32, general+nb+f32.  The negative binomial's step minus the Poisson's is what the
dispersion pass (csrc/count.hpp count_disp_partial / count_disp_finish), the sp(u) plane and rho's lgamma terms add.
The method of tools/realx_time.py: each configuration is a captured 16-step train graph timed with device events after a warm-up;
the configurations alternate over the rounds in one process; per configuration the median and the min - max spread:
    python tools/count_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--S 1] [--steps 16] [--launches 4] [--rounds 21] [--no-count]
--no-count leaves the two count configurations out (a library built from a commit without them: GMVAE_HIP_LIB=...).
Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("S", 1), ("steps", 16), ("launches", 4), ("rounds", 21)):
    ap.add_argument(f"--{k}", type=int, default=v)
ap.add_argument("--no-count", action="store_true")
a = ap.parse_args()
Lz, K, H, n, B, S = a.latent, a.K, a.hidden, a.steps, a.B, a.S

rng = np.random.default_rng(0)
grey = rng.integers(0, 256, size=(n, B, 784))
r = rng.random((n, B, 784))
grey[r < 0.3] = 0
grey[r >= 0.9] = 255
xbin = torch.from_numpy((grey > 127).astype(np.uint8)).cuda()
xb = torch.from_numpy(grey.astype(np.uint8)).cuda()
xf = torch.from_numpy(grey.astype(np.float32) / np.float32(255)).cuda()      # (the same t, as floats)
xc = torch.from_numpy(np.floor(grey.astype(np.float32) / 8)).cuda()          # (counts 0 .. 31, a third of them 0)

GA = dict(likelihood="gaussian", likelihood_sigma=0.25)
CONFIGS = {"bernoulli_general": (dict(clip_norm=float("inf")), xbin), "gauss_bytes": (GA, xb),
           "gauss_f32_lsig": (dict(real_valued=True, likelihood_scale="learned", **GA), xf)}
if not a.no_count:
    CONFIGS.update(poisson=(dict(likelihood="poisson"), xc), negative_binomial=(dict(likelihood="negative_binomial"), xc))


def capture(kw, x):
    e = Engine("gmvae", 784, Lz, K, [H], n_samples=S, random_seed=0, **kw)
    sched = L.step_schedule(e.dims(B), e.model)
    sx, replay = e.capture_train_step(B, lr=1e-3, n_steps=n)
    sx.copy_(x)
    replay()                                                               # warm-up
    torch.cuda.synchronize()
    return e, replay, sched


graphs = {name: capture(kw, x) for name, (kw, x) in CONFIGS.items()}
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
res = {"lib": os.path.basename(os.path.dirname(L.LIB_PATH)), "latent": Lz, "K": K, "hidden": H, "B": B, "S": S, "steps_per_graph": n,
       "launches": a.launches, "rounds": a.rounds, "step_us": {}, "min_us": {}, "max_us": {}, "schedules": {}, "losses": {}}
for name, (e, replay, sched) in graphs.items():
    tail = replay.tail_log[-1].double()
    res["step_us"][name] = round(float(np.median(times[name])), 2)
    res["min_us"][name] = round(float(np.min(times[name])), 2)
    res["max_us"][name] = round(float(np.max(times[name])), 2)
    res["schedules"][name] = sched
    res["losses"][name] = float((tail[0] / tail[4]).item())
st = res["step_us"]
if not a.no_count:
    res["nb_minus_poisson_us"] = round(st["negative_binomial"] - st["poisson"], 2)
    res["poisson_minus_gauss_bytes_us"] = round(st["poisson"] - st["gauss_bytes"], 2)
res["finite"] = bool(all(np.isfinite(list(res["losses"].values()))))
print(json.dumps(res), flush=True)
for name, (e, _, _) in graphs.items():
    e.drop_graphs()
