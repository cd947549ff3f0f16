"""Time of Engine.aggregate_posterior (include/gmvae_hip.h gmvae_mixture_logpdf_*: the aggregate posterior's log-densities at one
sample per example) at N = M examples, on the GMVAE (K = 10, L = 64) and the VAE_GMP at their default sizes, with per_dim on and
off, against a chunked torch implementation of the same statement on the same device, same encoders and same samples -- what a
user would otherwise write: [1024 queries, 1024 components, L] blocks, a running logaddexp per output.  The torch side computes
the aggregate posterior's three outputs only (no prior, no sampling).  Device events after a warm-up, alternating rounds:
    python tools/aggpost_time.py [N] [rounds] [reps] [torch_reps]
(default N = 10,000, 5 rounds of 3 calls; 1 torch call per round).  Prints one JSON line."""
import json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd.engine import Engine

a = sys.argv[1:]
N, rounds, reps, treps = (int(v) for v in (a[:4] + ["10000", "5", "3", "1"][len(a[:4]):]))
K, Lz, BLK = 10, 64, 1024
x = torch.from_numpy((np.random.default_rng(0).random((N, 784)) < 0.87).astype(np.uint8)).cuda()


@torch.no_grad()
def torch_aggregate(e, z, per_dim, chunk=Engine.AGG_CHUNK):
    """log q(z) [M], log q(z_d) [M, L] and log q(z | x_own) [M] of the engine's aggregate posterior at z, in fp32 torch."""
    M, Kc = z.shape[0], (e.K if e.model_name == "gmvae" else 1)
    ninf = dict(fill_value=-math.inf, dtype=torch.float32, device=z.device)
    joint, own, dim = torch.full((M,), **ninf), torch.full((M,), **ninf), (torch.full((M, Lz), **ninf) if per_dim else None)
    owner = torch.arange(M, device=z.device)
    for n0 in range(0, N, chunk):
        logpi, mu, sigma = e._latent_components(x[n0:n0 + chunk])
        logw, lsig = logpi.reshape(-1), sigma.log() + 0.5 * math.log(2 * math.pi)
        comp_owner = n0 + torch.arange(mu.shape[0], device=z.device) // Kc
        for m0 in range(0, M, BLK):
            zs = z[m0:m0 + BLK, None, :]
            for c0 in range(0, mu.shape[0], BLK):
                c = slice(c0, c0 + BLK)
                r = (zs - mu[None, c]) / sigma[None, c]
                t = -0.5 * r * r - lsig[None, c]
                s = logw[None, c] + t.sum(dim=2)
                joint[m0:m0 + BLK] = torch.logaddexp(joint[m0:m0 + BLK], torch.logsumexp(s, dim=1))
                mine = comp_owner[None, c] == owner[m0:m0 + BLK, None]
                if bool(mine.any()):
                    so = torch.logsumexp(s.masked_fill(~mine, -math.inf), dim=1)
                    own[m0:m0 + BLK] = torch.logaddexp(own[m0:m0 + BLK], so)
                if per_dim:
                    dim[m0:m0 + BLK] = torch.logaddexp(dim[m0:m0 + BLK], torch.logsumexp(logw[None, c, None] + t, dim=1))
    return joint - math.log(N), dim - math.log(N) if per_dim else None, own


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


out = {"N": N, "M": N, "L": Lz, "K": K, "rounds": rounds, "reps": reps, "torch_reps": treps, "torch_block": BLK}
for model in ("gmvae", "vae_gmp"):
    e = Engine(model, 784, Lz, K, [64], random_seed=0)
    z = e.aggregate_posterior(x, per_dim=False)["z"]
    fns = {}
    for pd in (True, False):
        tag = "per_dim" if pd else "joint"
        fns[f"hip_{tag}"] = (lambda pd=pd: e.aggregate_posterior(x, per_dim=pd), reps)
        if treps > 0:
            fns[f"torch_{tag}"] = (lambda pd=pd: torch_aggregate(e, z, pd), treps)
    for fn, _ in fns.values():                           # warm-up: workspaces, code objects, the caching allocator
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(rounds):                              # alternating rounds, the order swapped every round
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            ms[k].append(timed(*fns[k]))
    o = e.aggregate_posterior(x)
    comps = N * (K if model == "gmvae" else 1)
    res = {"components": comps, "triples": comps * N * Lz}
    for k, v in ms.items():
        res[f"{k}_ms"] = round(float(np.median(v)), 3)
        res[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
    if treps > 0:
        tj, td, to = torch_aggregate(e, o["z"], True)
        res["torch_over_hip_per_dim"] = round(res["torch_per_dim_ms"] / res["hip_per_dim_ms"], 2)
        res["torch_over_hip_joint"] = round(res["torch_joint_ms"] / res["hip_joint_ms"], 2)
        res["max_abs_diff_vs_torch"] = {"log_q_z": float((tj - o["log_q_z"]).abs().max()), "log_q_zd": float((td - o["log_q_zd"]).abs().max()),
                                        "log_q_zx": float((to - o["log_q_zx"]).abs().max())}
    res["per_dim_triples_per_s"] = round(res["triples"] / (res["hip_per_dim_ms"] * 1e-3))
    res.update(mi=float(o["mi"]), kl_marginal=float(o["kl_marginal"]), tc=float(o["tc"]), kl_avg=float(o["kl_avg"]),
               active_units=int(o["active_units"]),
               finite=bool(all(torch.isfinite(o[k]).all().item() for k in ("log_q_zx", "log_q_z", "log_q_zd", "log_p_z", "log_p_zd"))))
    out[model] = res
    del e
print(json.dumps(out), flush=True)
