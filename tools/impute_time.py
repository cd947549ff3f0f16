"""Time of the importance-sampling imputation (Engine.impute_posterior, include/gmvae_hip.h gmvae_impute) next to the bound it
rides on and next to a torch implementation of the same statement, configs[2] sizes (GMVAE, D 784, L 64, K 10, H 64), B = 1024,
missing rate 0.3, n = 500 samples:
    impute      Engine.impute_posterior(x, n, mask)                  -- the chunk passes of iw_bound + impute_merge + impute_fold
    iw_bound    Engine.iw_bound(x, n, mask=) at the same n and chunk -- the code the imputation adds its fold to
    torch       the same statement in chunked torch ops on the same device (fp32, torch's own noise): per chunk the three
                networks, the masked log w, a running max and the rescaled weighted sum of sigmoid(lambda)
The method of tools/pmask_time.py: device events after a warm-up, the configurations alternating in one process, per
configuration the median and the min - max spread over the rounds:
    python tools/impute_time.py [--latent 64] [--K 10] [--B 1024] [--hidden 64] [--n 500] [--chunk 0] [--draws 0] [--rounds 11]
Prints one JSON line; fold_us = impute - iw_bound and fold_share = fold_us / impute."""
import argparse, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import torch.nn.functional as F
from gmvae_amd.engine import Engine

ap = argparse.ArgumentParser()
for k, v in (("latent", 64), ("K", 10), ("B", 1024), ("hidden", 64), ("n", 500), ("chunk", 0), ("draws", 0), ("rounds", 11)):
    ap.add_argument(f"--{k}", type=int, default=v)
a = ap.parse_args()
Lz, K, H, B, n, D = a.latent, a.K, a.hidden, a.B, a.n, 784

rng = np.random.default_rng(0)
x = torch.from_numpy((rng.random((B, D)) < 0.87).astype(np.uint8)).cuda()
mask = torch.from_numpy((rng.random((B, D)) >= 0.3).astype(np.uint8)).cuda()
e = Engine("gmvae", D, Lz, K, [H], random_seed=0, pixel_mask=True)
chunk = a.chunk or max(1, min(n, e.IW_CHUNK_ROWS // B))
P = {k: v.detach() for k, v in e.views().items()}


def torch_impute():
    """The statement of tests/impute_ref.py in fp32 torch, chunk by chunk: (mean [B, D], bound [B])."""
    xf, mf = x.float(), (mask != 0).float()
    xm = xf * mf
    w = lambda net, i: (P[f"{net}_fcnet/linear_{i}/w"], P[f"{net}_fcnet/linear_{i}/b"])
    (wy0, by0), (wy1, by1) = w("encoder_y", 0), w("encoder_y", 1)
    (wg0, bg0), (wg1, bg1) = w("encoder_gmm", 0), w("encoder_gmm", 1)
    (wd0, bd0), (wd1, bd1) = w("decoder", 0), w("decoder", 1)
    wp, bp = w("prior_gmm", 0)
    c, smin, T = e.hp["raw_sigma_bias"], e.hp["sigma_min"], e.temperature
    logits = torch.relu(xm @ wy0 + by0) @ wy1 + by1
    lnq = torch.log_softmax(logits, dim=1)
    nent = (lnq.exp() * lnq).sum(dim=1)
    gx = xm @ wg0[:D] + bg0                                   # (the x part of encoder_gmm's first layer: once per batch)
    m_run = torch.full((B,), -math.inf, device="cuda")
    s1 = torch.zeros(B, device="cuda")
    acc = torch.zeros(B, D, device="cuda")
    for s0 in range(0, n, chunk):
        S = min(chunk, n - s0)
        u = torch.rand(B, S, K, device="cuda").clamp_min(1.2e-38)
        y = torch.softmax((logits[:, None, :] - torch.log(-torch.log(u))) / T, dim=2)
        pp = y @ wp + bp
        qp = torch.relu(gx[:, None, :] + y @ wg0[D:]) @ wg1 + bg1
        mu_q, sig_q = qp[..., :Lz], F.softplus(qp[..., Lz:] + c).clamp_min(smin)
        mu_p, sig_p = pp[..., :Lz], F.softplus(pp[..., Lz:] + c).clamp_min(smin)
        eps = torch.randn(B, S, Lz, device="cuda")
        z = mu_q + sig_q * eps
        logq = (-0.5 * eps * eps).sum(dim=2) - sig_q.log().sum(dim=2)
        logp = (-0.5 * ((z - mu_p) / sig_p) ** 2).sum(dim=2) - sig_p.log().sum(dim=2)
        lam = torch.relu(z @ wd0 + bd0) @ wd1 + bd1 + e.hp["gen_bias_init"]
        logpx = (mf[:, None, :] * (xf[:, None, :] * lam - F.softplus(lam))).sum(dim=2)
        lw = logpx + logp - logq - nent[:, None]
        m_new = torch.maximum(m_run, lw.max(dim=1).values)
        f, wgt = torch.exp(m_run - m_new), torch.exp(lw - m_new[:, None])
        acc = acc * f[:, None] + torch.einsum("bs,bsd->bd", wgt, torch.sigmoid(lam))
        s1 = s1 * f + wgt.sum(dim=1)
        m_run = m_new
    return acc / s1[:, None], m_run + s1.log() - math.log(n)


RUNS = {"impute": lambda: e.impute_posterior(x, n, mask=mask, n_draws=a.draws, chunk=chunk),
        "iw_bound": lambda: e.iw_bound(x, n, chunk=chunk, mask=mask),
        "torch": torch_impute}
outs = {}
for name, fn in RUNS.items():                                # warm-up: code objects, workspaces, torch's kernels
    for _ in range(2):
        outs[name] = fn()
torch.cuda.synchronize()
times = {name: [] for name in RUNS}
for _ in range(a.rounds):
    for name, fn in RUNS.items():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times[name].append(t0.elapsed_time(t1) * 1e3)
res = {"latent": Lz, "K": K, "hidden": H, "B": B, "n": n, "chunk": chunk, "draws": a.draws, "rounds": a.rounds,
       "call_us": {k: round(float(np.median(v)), 1) for k, v in times.items()},
       "min_us": {k: round(float(np.min(v)), 1) for k, v in times.items()},
       "max_us": {k: round(float(np.max(v)), 1) for k, v in times.items()}}
c = res["call_us"]
res["fold_us"] = round(c["impute"] - c["iw_bound"], 1)
res["fold_share"] = round((c["impute"] - c["iw_bound"]) / c["impute"], 3)
res["torch_over_impute"] = round(c["torch"] / c["impute"], 2)
# the three agree on what they compute: the same bound bits from the two library calls, the torch mean within Monte Carlo noise
res["bound_bits_equal"] = bool(torch.equal(outs["impute"]["bound"], outs["iw_bound"]["bound"]))
res["mean_abs_diff_torch"] = float((outs["impute"]["mean"] - outs["torch"][0]).abs().mean().item())
res["mean_ess"] = float(outs["impute"]["ess"].mean().item())
print(json.dumps(res), flush=True)
