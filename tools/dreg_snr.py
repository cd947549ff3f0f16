"""Signal-to-noise ratio of the inference network's gradient under the two estimators (Engine(grad_estimator=...),
include/gmvae_hip.h GMVAE_GRAD_DREG): per estimator and per S in {1, 5, 50}, |mean| / std over the noise of every coordinate of
the encoder's last-layer weight gradient, over 256 Philox steps at fixed parameters and data (the step counter keys the noise;
no optimizer step is taken), reported as the median over the coordinates -- for the GMVAE with y summed out
(y_inference="marginal_iw") at configs[2] sizes and for the VAE_GMP at configs[1] sizes:
    python tools/dreg_snr.py [--steps 256] [--samples 1,5,50] [--only gmvae|vae_gmp] [--B_gmvae 1024] [--B_gmp 256]
Rainforth et al. 2018 predict an SNR falling like 1/sqrt(S) for the standard estimator, Tucker et al. 2018 one rising like
sqrt(S) for the doubly reparameterised one.  Prints one JSON line."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import _lib as L
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--samples", default="1,5,50")
ap.add_argument("--only", default=None)
ap.add_argument("--B_gmvae", type=int, default=1024)
ap.add_argument("--B_gmp", type=int, default=256)
a = ap.parse_args()
SS = [int(s) for s in a.samples.split(",")]
FAMILIES = {"gmvae": ("gmvae", a.B_gmvae, dict(y_inference="marginal_iw"), "encoder_gmm_fcnet/linear_1/w"),
            "vae_gmp": ("vae_gmp", a.B_gmp, dict(), "encoder_fcnet/linear_1/w")}
if a.only:
    FAMILIES = {a.only: FAMILIES[a.only]}
res = {"steps": a.steps, "samples": SS, "snr_median": {}, "snr_mean": {}, "schedules": {}, "coords": {}}
for fam, (model, B, kw, wname) in FAMILIES.items():
    x = torch.from_numpy((np.random.default_rng(0).random((B, 784)) < 0.87).astype(np.uint8)).cuda()
    for S in SS:
        for est in L.GRAD_ESTIMATORS:
            e = Engine(model, 784, 64, 10, [64], n_samples=S, random_seed=0, grad_estimator=est, **kw)
            off, shape = next((o, s) for n, s, o in e.layout if n == wname)
            k = shape[0] * shape[1]
            s1 = torch.zeros(k, dtype=torch.float64, device="cuda")
            s2 = torch.zeros(k, dtype=torch.float64, device="cuda")
            for t in range(a.steps):
                e.global_step = t
                g = e.step(x)[off:off + k].double() / B
                s1 += g
                s2 += g * g
            torch.cuda.synchronize()
            mean = s1 / a.steps
            var = (s2 / a.steps - mean * mean).clamp_min(0) * (a.steps / (a.steps - 1))
            ok = var > 0
            snr = (mean[ok].abs() / var[ok].sqrt()).cpu().numpy()
            key = f"{fam}_S{S}_{est}"
            res["snr_median"][key] = float(np.median(snr))
            res["snr_mean"][key] = float(np.mean(snr))
            res["coords"][key] = int(ok.sum().item())
            res["schedules"][key] = L.step_schedule(e.dims(B), e.model)
            del e
            torch.cuda.empty_cache()
print(json.dumps(res), flush=True)
