#!/usr/bin/env python
"""ELBO-samples/sec of the GMVAE training step on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A step = noise (Philox) + forward + backward + (RCCL all-reduce of the flat
[P+8] gradient buffer when N>1) + TF-Adam, on a synthetic MNIST-shaped uint8
batch already resident in HBM.  Workload = BASELINE.json configs[2]/[3]:
GMVAE, D=784, K=10, latent 64, batch 1024 PER GPU (weak scaling: 8 GPUs = the
B=8192 config), hidden = the reference default 64 (scripts/run_gmvae.py:19).
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline line.
--full adds everything else: parity against the fp64 oracle, the CPU baseline,
repeated regions, HIP-event and roofline figures, the data-parallel timeline.
--dump-outputs DIR writes what the last timed step computed (dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_HBM_GBS = 8000.0
PLANES_EXACT = os.environ.get("GMVAE_PLANES_EXACT", "0") not in ("", "0")       # the plane GEMMs' piece form (gmvae_hip.hip run_step)
PLANE_PIECES = 6.0 if PLANES_EXACT else 3.0
PLANES_DTYPE = ("f32 (products as 6 exact bf16 piece products, fp32 accumulation)" if PLANES_EXACT else
                "f32 (products as 3 f16 piece products of scaled pairs: <= 3 x 2^-22 per product; fp32 accumulation)")
PEAK_BF16_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 peak (v_mfma_f32_32x32x16_bf16)


# Named workloads (per-GPU shapes).  configs0..2 = BASELINE.json configs[0..2]; configs4_shard = the per-GPU shard of
# configs[4] (B = 4096 / 8); run_train = the reference's bin/run_train.sh sizes.  Multi-GPU runs of configs2 ARE configs[3].
CONFIGS = {
    "configs0": dict(model="vae", batch=100, latent=2, components=1, hidden=64, layers=1, data_dim=784, n_samples=1),
    "configs1": dict(model="vae_gmp", batch=256, latent=64, components=10, hidden=64, layers=1, data_dim=784, n_samples=1),
    "configs2": dict(model="gmvae", batch=1024, latent=64, components=10, hidden=64, layers=1, data_dim=784, n_samples=1),
    "configs4_shard": dict(model="gmvae", batch=512, latent=64, components=64, hidden=512, layers=1, data_dim=3072, n_samples=50),
    "run_train": dict(model="gmvae", batch=64, latent=128, components=10, hidden=512, layers=1, data_dim=784, n_samples=1),
    # H = 512 (bin/run_train.sh:6) is the "realistic point" of configs[1] / configs[2]
    "configs1_h512": dict(model="vae_gmp", batch=256, latent=64, components=10, hidden=512, layers=1, data_dim=784, n_samples=1),
    "configs2_h512": dict(model="gmvae", batch=1024, latent=64, components=10, hidden=512, layers=1, data_dim=784, n_samples=1),
    # one rank's step of BASELINE configs[3] (1024 rows per GPU) on the DATA-PARALLEL path with a one-rank RCCL communicator:
    # gradients -> RCCL all-reduce node inside the hipGraph (an identity copy here) -> TF-Adam scaled by 1/count.  What the
    # path costs before a byte crosses xGMI; `--gpus N` runs the same path with N ranks.
    # the forward-only evaluation of BASELINE.json's metric: the -log p(x) importance-weighted bound at S = 50 samples per row
    # on configs[2]'s model and batch (scripts/runners.py:324-333 reuses the model's loss for evaluation): 51,200 sample rows
    "eval_iwae": dict(model="gmvae", batch=1024, latent=64, components=10, hidden=64, layers=1, data_dim=784, n_samples=50,
                      eval_only=True),
    # the same bound for BASELINE configs[1]'s and configs[0]'s models at their batches (csrc/evalf.hpp evalf_rows_v)
    "eval_iwae_vae_gmp": dict(model="vae_gmp", batch=256, latent=64, components=10, hidden=64, layers=1, data_dim=784, n_samples=50,
                              eval_only=True),
    "eval_iwae_vae": dict(model="vae", batch=100, latent=2, components=1, hidden=64, layers=1, data_dim=784, n_samples=50,
                          eval_only=True),
    "configs3_dp1": dict(model="gmvae", batch=1024, latent=64, components=10, hidden=64, layers=1, data_dim=784, n_samples=1,
                         dp_world1=True),
}


def workload_name(a, n_gpus):
    key = dict(model=a.model, batch=a.batch, latent=a.latent, components=a.components if a.model != "vae" else 1,
               hidden=a.hidden, layers=a.layers, data_dim=a.data_dim, n_samples=a.n_samples)
    if getattr(a, "dp_world1", False) and n_gpus == 1:
        return "one rank of BASELINE configs[3] on the data-parallel path (one-rank RCCL communicator)"
    for name, c in CONFIGS.items():
        if {k: v for k, v in c.items() if k not in ("dp_world1", "eval_only")} == key and not c.get("eval_only"):
            if name == "configs2":
                return "BASELINE configs[2]" if n_gpus == 1 else f"BASELINE configs[3] shape: 1024 rows per GPU x {n_gpus}"
            return {"configs0": "BASELINE configs[0]", "configs1": "BASELINE configs[1]",
                    "configs4_shard": "per-GPU shard of BASELINE configs[4]", "run_train": "bin/run_train.sh sizes",
                    "configs1_h512": "BASELINE configs[1] at hidden 512", "configs2_h512": "BASELINE configs[2] at hidden 512"}[name]
    return "custom sizes"


def self_launch(a):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start the N ranks ourselves, BEFORE anything
    touches the GPU (one process per GPU over RCCL, the same command line the driver uses), and exit with their code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--model", default="gmvae", choices=["gmvae", "vae", "vae_gmp"])
    ap.add_argument("--batch", type=int, default=1024, help="per-GPU batch")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--data-dim", type=int, default=784)
    ap.add_argument("--n-samples", type=int, default=1)
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of one hipGraph per step")
    ap.add_argument("--pipeline", action="store_true",
                    help="start every step from raw uint8 pixels resident in HBM: the reference's dynamic binarisation "
                         "(gmvae_binarize) runs inside the train graph (single GPU)")
    ap.add_argument("--graph-steps", type=int, default=40, help="consecutive steps captured in one hipGraph launch")
    ap.add_argument("--allow-fallback", action="store_true",
                    help="N > 1: accept a slower data-parallel path (eager C-side step or torch.distributed all-reduce) when "
                         "the RCCL all-reduce cannot be captured inside the hipGraph; without it such a run exits non-zero")
    ap.add_argument("--safe-schedule", action="store_true",
                    help="start on the schedule without waits between the workgroups of a launch (GMVAE_SCHED_SAFE): what a run "
                         "that shares its GPU needs (tests: two ranks on one device)")
    ap.add_argument("--full", action="store_true",
                    help="measure and check beyond the headline figure: parity against the fp64 oracle, the CPU baseline, "
                         "repeated short regions, per-launch HIP events and roofline, the data-parallel timeline, the exact-"
                         "triples step time and the replicas' checksum")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32, <= 64 MB in "
                         "all); on one GPU the same arguments give the same inputs in every run")
    ap.add_argument("--no-iwae-bound", action="store_true", help="--full: skip the -log p(x) IWAE bound (S = 50) of the parity block")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--levels", action="store_true", help="--full: also print the per-launch table to stderr")
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="a named workload (BASELINE.json configs / SURVEY.md 8(d)); the default line is configs2")
    ap.add_argument("--dp-world1", action="store_true",
                    help="N = 1 on the data-parallel path: RCCL all-reduce node (one-rank communicator) inside the hipGraph")
    a = ap.parse_args()
    if a.config:
        for k, v in CONFIGS[a.config].items():
            setattr(a, k, v)
    return a


DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array, flattened, as out_dir/<name>.npy in float32, DUMP_BYTES in all at most.  The budget is split
    evenly; an array larger than its share keeps a fixed sample of its elements (np.random.default_rng(0), sorted flat
    indices): the same from run to run."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for k, v in arrays.items()}
    left = (DUMP_BYTES - 4096) // 4                        # elements (room for the .npy headers)
    for i, (name, v) in enumerate(sorted(arrays.items(), key=lambda kv: kv[1].size)):
        n = min(v.size, left // (len(arrays) - i))
        if n < v.size:
            v = v[np.sort(np.random.default_rng(0).choice(v.size, n, replace=False))]
        left -= n
        np.save(os.path.join(out_dir, f"{name}.npy"), v)


def cpu_thread_counts():
    """BLAS thread counts worth timing: 1 (the reference pins intra_op = inter_op = 1, scripts/runners.py:203-204), a few
    small pools, and the PHYSICAL cores this process may use -- never the logical count: round 2's "all 256 cores" leg was
    4.5x slower than one thread (SMT siblings + 256 threads on 64-wide GEMMs = oversubscription, not a baseline)."""
    logical = len(os.sched_getaffinity(0))
    try:
        import psutil
        phys_all, log_all = psutil.cpu_count(logical=False) or logical, psutil.cpu_count(logical=True) or logical
        physical = max(1, min(logical, logical * phys_all // max(log_all, 1)))
    except Exception:
        physical = logical
    return sorted({1, 4, 8, 16, physical} & set(range(1, physical + 1))), logical, physical


def cpu_baseline(model, dims, B, flat, x, eps, u, budget_s):
    """CPU leg, part 2: the oracle's fp32 restatement of the SAME step (fwd+bwd+TF-Adam) timed on the host cores, at each
    thread count of cpu_thread_counts(); returns {threads: (samples/s, steps)} and the core counts."""
    import oracle as O
    d = O.Dims(**dims)
    model_id = O.MODEL_NAMES[model]
    res = {}
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        threadpool_limits = None
    counts, logical, physical = cpu_thread_counts()
    if threadpool_limits is None:
        counts = [1]                                   # (cannot bound the BLAS pool: report what one thread... is not knowable)
    import contextlib
    for nthreads in counts:
        ctx = threadpool_limits(limits=nthreads) if threadpool_limits else contextlib.nullcontext()
        with ctx:
            f, m, v = flat.copy(), np.zeros_like(flat), np.zeros_like(flat)
            O.train_step(model_id, d, f, m, v, 1, x, eps, u, dtype=np.float32)      # warm
            t0, n = time.perf_counter(), 0
            while time.perf_counter() - t0 < budget_s / len(counts) and n < 200:
                f, m, v, _, _ = O.train_step(model_id, d, f, m, v, n + 1, x, eps, u, dtype=np.float32)
                n += 1
            dt = time.perf_counter() - t0
            res[nthreads] = (B * d.S * n / dt, n)
    return res, logical, physical


def flops_per_step(model: str, D: int, L: int, K: int, hidden, S: int, B: int) -> float:
    """SURVEY.md A.1 FLOP rule: 2*(fwd + dW + dX MACs) per sample, the x-input dX excluded (it is never computed)."""
    def mac(n_in, n_out):
        dims = [n_in] + list(hidden) + [n_out]
        return sum(p * q for p, q in zip(dims[:-1], dims[1:]))
    h0 = hidden[0]
    if model == "gmvae":
        fwd = mac(D, K) + S * (K * 2 * L + mac(D + K, 2 * L) + mac(L, D))
        dx = fwd - D * h0 * (1 + S)
    else:
        fwd = mac(D, 2 * L) + S * mac(L, D)
        dx = fwd - D * h0
    return 2.0 * B * (2 * fwd + dx)


def cpu_parity(model: str, dims: dict, flat0, x_np, eps_np, u_np):
    """CPU leg, part 1 (the checker): ELBO of the fp64 oracle on the inputs the HIP step just ran on."""
    import oracle as O
    d = O.Dims(**dims)
    mid = O.MODEL_NAMES[model]
    C64 = O.forward(mid, d, O.unpack(mid, d, flat0.astype(np.float64)), x_np, eps_np, u_np, np.float64)
    return float(-C64["loss"])


def flops_forward(model: str, D: int, L: int, K: int, hidden, S: int, B: int) -> float:
    """2 * forward MACs of one evaluation: the layers over x once per batch row, everything else per sample row."""
    def mac(n_in, n_out):
        dims = [n_in] + list(hidden) + [n_out]
        return sum(p * q for p, q in zip(dims[:-1], dims[1:]))
    h0 = hidden[0]
    if model == "gmvae":
        per_row = mac(D, K) + D * h0                         # encoder_y, and encoder_gmm's x rows of its first layer
        per_sample = K * 2 * L + (mac(D + K, 2 * L) - D * h0) + mac(L, D)
    else:
        per_row, per_sample = mac(D, 2 * L), mac(L, D)
    return 2.0 * B * (per_row + S * per_sample)


def main_eval(a):
    """--config eval_iwae: throughput of the forward-only -log p(x) bound (gmvae_forward, S importance samples per row, in-kernel
    Philox noise) -- ONE JSON line with the same keys as the training line; a "step" is one evaluation pass over the batch."""
    import torch
    from gmvae_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    if a.gpus != 1:
        raise SystemExit("bench.py --config eval_iwae: evaluation batches are independent -- run one process per GPU (replicas only)")
    torch.cuda.set_device(0)
    hidden = [a.hidden] * a.layers
    K = a.components if a.model != "vae" else 1
    S, B, D, Lz = a.n_samples, a.batch, a.data_dim, a.latent
    dims = dict(D=D, L=Lz, K=K, hidden=tuple(hidden), S=S)
    eng = Engine(a.model, D, Lz, K, hidden, n_samples=S, random_seed=0)
    x_np = (np.random.default_rng(1234).random((B, D)) < 0.87).astype(np.uint8)
    x = torch.from_numpy(x_np).cuda()
    flat0 = eng.params.detach().cpu().numpy()
    parity = None
    if a.full:
        # ---- parity: the bound on a seeded batch of <= 256 rows, HIP forward vs the fp64 oracle on identical (x, eps, u)
        tiny = float(np.finfo(np.float32).tiny)
        B_iw = max(8, min(256, B, int(2e7 // (D * S))))
        rn = np.random.default_rng(4242)
        eps_iw = rn.standard_normal((B_iw * S, Lz)).astype(np.float32)
        u_iw = None
        if a.model == "gmvae":
            u_iw = np.clip(rn.uniform(tiny, 1.0, (B_iw * S, K)).astype(np.float32), tiny, np.nextafter(np.float32(1), np.float32(0)))
        fw = eng.forward(x[:B_iw], torch.from_numpy(eps_iw), None if u_iw is None else torch.from_numpy(u_iw), n_samples=S)
        torch.cuda.synchronize()
        t_iw = fw["tail"].cpu().numpy().astype(np.float64)
        iw_hip = float(t_iw[0] / t_iw[4])
        iw_cpu = -cpu_parity(a.model, dims, flat0, x_np[:B_iw], eps_iw, u_iw)
        parity = {"neg_log_px_bound_hip": iw_hip, "neg_log_px_bound_cpu_fp64": iw_cpu, "n_samples": S, "rows": B_iw,
                  "rel_err": float(abs(iw_hip - iw_cpu) / abs(iw_cpu))}
    # ---- timing: W + K passes of ONE captured forward replayed back to back (HIP events on the launch stream)
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.75:                 # (DVFS: the host-side oracle above let the clocks drop)
        eng.profile_forward(x, n_samples=S, iters=20)
    eng.profile_forward(x, n_samples=S, iters=max(1, a.warmup))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    levels, us_total, tail = eng.profile_forward(x, n_samples=S, iters=a.steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0                           # (includes the per-launch pass: not the figure of merit)
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {"loss_terms": tail.cpu().numpy()})     # the last pass's [TAIL] loss sums
    dt_ms = us_total * 1e-3
    value = B * S / (us_total * 1e-6)
    fl_alg = flops_forward(a.model, D, Lz, K, hidden, S, B)
    gem = [l for l in levels if l[2] > 0]
    dom = max(gem, key=lambda l: l[1])
    from gmvae_amd import _lib as LIB
    roof = {"bound": "mfma", "kernel": dom[0] if dom[0].startswith(("mega", "sk_", "dw_", "rows_", "first_", "evalf")) else f"gemm_grouped<{dom[0]}>",
            "achieved": dom[2] / dom[1] * 1e-6, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": dom[2] / dom[1] * 1e-6 / PEAK_F32_MFMA_TFLOPS, "traffic": None,
            "usec_per_launch": dom[1], "flops_per_launch": dom[2],
            "timing": "per launch: hipEvents around eager launches (mean); the pass: captured forward passes replayed back to back (passes_per_graph_launch per launch)",
            "step_flops_alg": fl_alg, "step_tflops_alg": fl_alg / us_total * 1e-6,
            "step_frac_of_mfma_peak": fl_alg / us_total * 1e-6 / PEAK_F32_MFMA_TFLOPS,
            "step_flops_executed": sum(l[2] for l in levels), "launches_per_step": len(levels),
            "sum_launch_usec": sum(l[1] for l in levels),
            "levels": [[nm, round(us, 2), round(f / max(us, 1e-9) * 1e-6, 2)] for nm, us, f in levels],
            "levels_columns": ["launch", "usec (events, eager)", "TFLOP/s"],
            "schedule": LIB.step_schedule(eng.dims(B, S), eng.model) + " (forward only)"}
    # forward-only passes at thousands of rows run the logits GEMM on f16 pairs (gmvae_hip.hip fwd_pairs_ok): the pass then carries
    # a "split_planes" level, and the launch is priced against the instruction it issues (three piece products per product)
    fwd_pairs = any(l[0] == "split_planes" for l in levels) and dom[0] == "fwd_dec_bernoulli"
    if fwd_pairs:
        pk = PEAK_BF16_MFMA_TFLOPS / PLANE_PIECES
        roof.update({"peak": pk, "frac": roof["achieved"] / pk, "piece_products_per_product": PLANE_PIECES,
                     "peak_note": f"dense f16 MFMA peak 2500 TFLOP/s / {PLANE_PIECES:.0f} piece products per fp32 product; fp32 accumulation; "
                                  "K = 64 is four 16-deep rounds per tile: the launch is its Bernoulli epilogue's vector work",
                     "frac_of_f32_mfma_peak": roof["achieved"] / PEAK_F32_MFMA_TFLOPS})
    if dom[0] in ("evalf_rows", "evalf_rows_v"):
        # the one-launch evaluation (csrc/evalf.hpp): the output layer (64 -> D per sample row) multiplies as exact bf16 piece products
        # (6 per fp32 product), the small layers as fp32 MFMA: priced against the time the two parts would take at their own peaks
        f_top = 2.0 * B * S * (hidden[-1] * D + (hidden[0] * 2 * Lz if a.model == "gmvae" else 0) + (Lz * hidden[0] if Lz >= 16 else 0))   # output layer, q head, decoder hidden layer
        f_small = dom[2] - f_top
        t_ideal = f_small / (PEAK_F32_MFMA_TFLOPS * 1e6) + f_top / (PEAK_BF16_MFMA_TFLOPS / 6.0 * 1e6)      # us
        pk = dom[2] / t_ideal * 1e-6
        roof.update({"peak": pk, "frac": roof["achieved"] / pk, "frac_of_f32_mfma_peak": roof["achieved"] / PEAK_F32_MFMA_TFLOPS,
                     "piece_products_per_product": 6.0,
                     "peak_note": f"blended: {f_top / dom[2]:.0%} of the launch's FLOPs (the decoder's two layers and the q head) run as 6 exact bf16 piece products per "
                                  f"fp32 product (dense bf16 peak 2500 / 6 = 416.7 fp32-equivalent TFLOP/s), the rest as fp32 MFMA (157.3): "
                                  f"ideal {t_ideal:.1f} us; measured (tools/evstamps.py): matrix and vector instructions of this kernel do not "
                                  "overlap -- the dense 4-pass bf16 MFMAs leave no issue shadow -- so its time is the SUM of both"})
        if os.environ.get("GMVAE_EVAL_GRAPH_PASSES"):
            roof["passes_per_graph_launch"] = int(os.environ["GMVAE_EVAL_GRAPH_PASSES"])
        else:
            roof["passes_per_graph_launch"] = min(8, a.steps)
    try:
        import csv, glob
        stats = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_eval_iwae_kernel_stats.csv")))
        if stats:
            roof["rocprof_source"] = os.path.relpath(stats[-1], ROOT)
            want = "void gmvae::gemm_grouped<gmvae::Cfg<128, 128, 32, 2, 2, 1, 2>, %d>" % (3 if fwd_pairs else 0)
            if dom[0] in ("evalf_rows", "evalf_rows_v"):
                want = "void gmvae::evalf_rows<0>" 
            for row in csv.DictReader(open(stats[-1])):
                if row["Name"].startswith(want):
                    roof["rocprof_usec_per_launch"] = float(row["AverageNs"]) * 1e-3
                    roof["frac_rocprof"] = dom[2] / roof["rocprof_usec_per_launch"] * 1e-6 / roof["peak"]
                    break
    except Exception:
        pass
    cpu = None
    if a.full and not a.no_cpu_baseline:
        import oracle as O
        d_o = O.Dims(**dims)
        mid = O.MODEL_NAMES[a.model]
        pr32 = O.unpack(mid, d_o, flat0.astype(np.float32))
        nb = B_iw
        n_done, t1 = 0, time.perf_counter()
        while time.perf_counter() - t1 < a.cpu_seconds or n_done == 0:
            O.forward(mid, d_o, pr32, x_np[:nb], eps_iw, u_iw, np.float32)
            n_done += 1
        el = time.perf_counter() - t1
        cpu = {"value": nb * S * n_done / el, "unit": "ELBO-samples/sec", "cores": "default BLAS threads", "kind": "port",
               "sample": f"{n_done} forward passes of the fp32 NumPy/BLAS oracle over {nb} rows x {S} samples in {el:.1f} s"}
    out = {"metric": "ELBO-samples/sec", "value": value, "unit": "samples/sec", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": dt_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": PLANES_DTYPE if fwd_pairs else "f32", "data": "synthetic",
           "config": {"workload": f"{a.model} forward-only -log p(x) IWAE bound (gmvae_forward, in-kernel Philox noise), D={D} K={K} "
                                  f"L={Lz} hidden={hidden} S={S} samples per row, batch {B} = {B * S} sample rows "
                                  f"(BASELINE.json metric's bound on configs[2]'s model)",
                      "global_batch": B, "parallelism": "dp1", "hipgraph": True},
           "host_wall_seconds_of_the_profile_call": wall,
           "neg_log_px_bound_of_the_timed_batch": float(tail[0].item() / max(tail[4].item(), 1.0)),
           "roofline": roof, "cpu_baseline": cpu, "parity": {"iwae_bound": parity} if parity else None}
    print(json.dumps(out), flush=True)


def main():
    a = parse()
    if getattr(a, "eval_only", False):
        return main_eval(a)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks")
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    # GMVAE_DIST_BACKEND=gloo: several ranks on ONE device (tests; RCCL refuses that) -- the all-reduce is then staged
    # through the host (gmvae_amd.parallel.all_reduce_flat) and the line says so (config.all_reduce, "fallback")
    backend = os.environ.get("GMVAE_DIST_BACKEND") or "nccl"
    local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    n_gpus = world
    dp = world > 1 or bool(a.dp_world1)              # the data-parallel path (also with ONE rank: --config configs3_dp1)

    def dev_all_reduce(t, op):                      # small control tensors: on the device over RCCL, through the host over gloo
        if backend == "nccl":
            dist.all_reduce(t, op=op)
            return t
        h = t.cpu()
        dist.all_reduce(h, op=op)
        return h.to(t.device)

    from types import SimpleNamespace
    from gmvae_amd.engine import Engine

    hidden = [a.hidden] * a.layers
    dims = dict(D=a.data_dim, L=a.latent, K=a.components if a.model != "vae" else 1, hidden=tuple(hidden), S=a.n_samples)
    d = SimpleNamespace(**dims)
    B = a.batch
    # random_seed=None is the reference's default (scripts/run_gmvae.py:30): every process seeds itself from entropy, so the
    # replicas START different; sync_replicas() makes rank 0's parameters, moments, step and noise seed everyone's.  The
    # noise itself differs per rank by construction: the Philox counter holds the GLOBAL row (rank * B + b).
    eng = Engine(a.model, d.D, d.L, d.K, hidden, n_samples=d.S, random_seed=0 if world == 1 else None)
    if a.safe_schedule:
        eng.use_safe_schedule()
    eng.sync_replicas()
    # synthetic MNIST-shaped batch: Bernoulli(0.87) uint8, per-rank shard of the global batch
    x_np = (np.random.default_rng(1234 + rank).random((B, d.D)) < 0.87).astype(np.uint8)
    x = torch.from_numpy(x_np).cuda()

    parity = {}
    if a.full:
        # ---- parity in the same run: HIP vs the fp64 CPU restatement on identical (x, eps, u, parameters)
        rn = np.random.default_rng(42)
        tiny = float(np.finfo(np.float32).tiny)
        eps_np = rn.standard_normal((B * d.S, d.L)).astype(np.float32)
        u_np = np.clip(rn.uniform(tiny, 1.0, (B * d.S, d.K)).astype(np.float32), tiny, np.nextafter(np.float32(1), np.float32(0)))
        if a.model != "gmvae":
            u_np = None
        flat0 = eng.params.detach().cpu().numpy()
        buf = eng.step(x, torch.from_numpy(eps_np), None if u_np is None else torch.from_numpy(u_np))
        torch.cuda.synchronize()
        tail = buf[eng.P:].cpu().numpy().astype(np.float64)
        elbo_hip = -tail[0] / tail[4]
    if a.full and rank == 0:
        elbo_cpu = cpu_parity(a.model, dims, flat0, x_np, eps_np, u_np)
        parity = {"elbo_hip": elbo_hip, "elbo_cpu_fp64": elbo_cpu, "rel_err": float(abs(elbo_hip - elbo_cpu) / abs(elbo_cpu))}
        if not a.no_iwae_bound:
            # BASELINE.json's metric also names the -log p(x) IWAE bound at K = 10: the S = 50 importance-weighted bound of the
            # same model (the step's parameters) on a fixed seeded batch of 256 rows, HIP forward path vs the fp64 oracle on
            # identical (x, eps, u).  A forward-only evaluation (gmvae_forward), outside the timed region.
            try:
                S_iw = 50
                B_iw = max(8, min(256, B, int(2e7 // (d.D * S_iw))))      # (bounds the oracle's share of the run to seconds)
                rn2 = np.random.default_rng(4242)
                eps_iw = rn2.standard_normal((B_iw * S_iw, d.L)).astype(np.float32)
                u_iw = None
                if a.model == "gmvae":
                    u_iw = np.clip(rn2.uniform(tiny, 1.0, (B_iw * S_iw, d.K)).astype(np.float32), tiny, np.nextafter(np.float32(1), np.float32(0)))
                fw = eng.forward(x[:B_iw], torch.from_numpy(eps_iw), None if u_iw is None else torch.from_numpy(u_iw), n_samples=S_iw)
                torch.cuda.synchronize()
                t_iw = fw["tail"].cpu().numpy().astype(np.float64)
                iw_hip = float(t_iw[0] / t_iw[4])
                iw_cpu = -cpu_parity(a.model, dict(dims, S=S_iw), flat0, x_np[:B_iw], eps_iw, u_iw)
                parity["iwae_bound"] = {"neg_log_px_bound_hip": iw_hip, "neg_log_px_bound_cpu_fp64": iw_cpu, "n_samples": S_iw,
                                        "rows": B_iw, "rel_err": float(abs(iw_hip - iw_cpu) / abs(iw_cpu)),
                                        "single_sample_neg_elbo_hip": -elbo_hip}
            except Exception as e:                  # (never let the secondary figure take the line down)
                parity["iwae_bound"] = {"error": f"{type(e).__name__}: {e}"}

    # ---- the timed loop
    use_graph = not a.no_graph
    fallbacks = []

    def fallback(why):
        """A slower data-parallel path than the one the line is supposed to measure.  The run GOES ON and the JSON line is
        printed either way -- with "fallback": true, the reasons, and config.all_reduce naming the path actually timed -- so
        that an unattended multi-GPU run can never return nothing; without --allow-fallback the process then exits non-zero.
        (Every decision that leads here is taken jointly by all ranks -- Engine._agree -- so they all take the same path.)"""
        fallbacks.append(why)
        if rank == 0:
            print(f"[bench] {why}", file=sys.stderr)

    if world > 1 and backend != "nccl":
        fallback(f"GMVAE_DIST_BACKEND={backend}: the all-reduce is staged through the host between two eager halves of the step")
    elif dp:
        try:
            eng.enable_rccl()           # RCCL communicator inside libgmvae_hip.so: step + all-reduce + Adam in one graph
        except Exception as e:
            fallback(f"in-library RCCL unavailable ({type(e).__name__}: {e}): torch.distributed all-reduce between two eager halves")
    # One graph launch runs G consecutive steps, each on its own resident batch (the next G batches of an input
    # pipeline): the GPU idles ~6 us between two graph launches, nothing between the kernels inside one.
    # (the largest divisor of K up to --graph-steps, so that the timed K steps are whole launches of one graph)
    G = max(g for g in range(1, max(1, min(a.graph_steps, a.steps)) + 1) if a.steps % g == 0)
    if G < 8 <= a.steps:                 # no useful divisor: whole launches of --graph-steps + single steps for the rest
        G = min(a.graph_steps, a.steps)
    multi_fn = None
    if use_graph:
        try:
            static_x, replay = eng.capture_train_step(B, lr=1e-3, all_reduce=dp)
            static_x.copy_(x)
            step_fn = replay
            if a.pipeline and world == 1:
                from gmvae_amd.data import DeviceDataset
                ds = DeviceDataset(np.random.default_rng(99).integers(0, 256, (60000, d.D), dtype=np.uint8), shuffle=True, seed=1)
                multi_fn = eng.capture_train_pipeline(ds, B, lr=1e-3, n_steps=G)
                step_fn = eng.capture_train_pipeline(ds, B, lr=1e-3, n_steps=1)
            elif G > 1:
                xs, multi_fn = eng.capture_train_step(B, lr=1e-3, all_reduce=dp, n_steps=G)
                rng = np.random.default_rng(4321 + rank)
                xs.copy_(torch.from_numpy((rng.random((G, B, d.D)) < 0.87).astype(np.uint8)))
        except Exception as e:                      # e.g. RCCL inside capture unsupported
            fallback(f"graph capture failed ({type(e).__name__}: {e}): eager launches")
            use_graph = False
            multi_fn = None
        if world > 1 and use_graph and getattr(eng, "dp_mode", None) != "rccl-in-hipgraph" and not fallbacks:
            fallback(f"the RCCL all-reduce was not captured inside the hipGraph (data-parallel mode: {getattr(eng, 'dp_mode', None)})")
    if not use_graph:
        def step_fn():
            eng.train_step(x, lr=1e-3, all_reduce=dp)

    def run_steps(k):                               # exactly k training steps
        if multi_fn is not None:
            for _ in range(k // G):
                multi_fn()
            k = k % G
        for _ in range(k):
            step_fn()

    # The GPU drops its clocks while the host runs the fp64 parity check above; a step is ~100 us, so W
    # warm-up steps alone can be shorter than the DVFS ramp (measured: 2x slower timed region).  Spin the
    # same step untimed for a fixed wall time first, THEN do the W warm-up steps the contract asks for.
    if world == 1:
        t_pre = time.perf_counter()
        while time.perf_counter() - t_pre < 0.75:
            run_steps(2 * G)
            torch.cuda.synchronize()
    else:
        # every rank must issue the SAME number of steps (each contains a collective): whole rounds of 2 G steps until
        # ANY rank's clock says 0.75 s (one all-reduced stop flag per round), at most 4000 steps
        t_pre, done = time.perf_counter(), 0
        while done < 4000:
            run_steps(2 * G)
            torch.cuda.synchronize()
            done += 2 * G
            stop = torch.tensor([1 if time.perf_counter() - t_pre >= 0.75 else 0], dtype=torch.int32, device="cuda")
            if bool(dev_all_reduce(stop, dist.ReduceOp.MAX).item()):
                break
    # Safety net for unattended runs: the 3-launch schedule's workgroups wait for each other inside mega_fwd_bwd and
    # need the whole chip.  If a wait ever timed out during the pre-warm (something else held CUs), every rank
    # switches to the schedule without mutual waits and re-captures -- slower, never stalling.
    bad = torch.tensor([eng.handoff_timeouts()], dtype=torch.int32, device="cuda")
    if world > 1:
        bad = dev_all_reduce(bad, dist.ReduceOp.MAX)
    safe_schedule = bool(bad.item())
    if safe_schedule and use_graph and not eng.safe_schedule:
        if rank == 0:
            print("[bench] a hand-off of the fused schedule timed out during the pre-warm (something else holds part of the "
                  "chip): switching to the schedule without mutual waits -- reported as config.safe_schedule", file=sys.stderr)
        eng.use_safe_schedule()
        eng.init_parameters(0)                       # poisoned steps were skipped by the optimizer, but start clean anyway
        eng.sync_replicas()
        static_x, step_fn = eng.capture_train_step(B, lr=1e-3, all_reduce=dp)
        static_x.copy_(x)
        multi_fn = None
        if G > 1:
            xs, multi_fn = eng.capture_train_step(B, lr=1e-3, all_reduce=dp, n_steps=G)
            xs.copy_(torch.from_numpy((np.random.default_rng(4321 + rank).random((G, B, d.D)) < 0.87).astype(np.uint8)))
        run_steps(2 * G)
        torch.cuda.synchronize()
    safe_schedule = bool(eng.safe_schedule)
    if world == 1:
        # the pre-warm runs for a wall time, not a step count: the W + K steps start again from the state the Engine was
        # created in (random_seed 0), so that the last step sees the same inputs in every run (--dump-outputs).  (A train graph
        # builds its weight images from the parameters at the first step of every launch: nothing stale survives this.)
        eng.init_parameters(0)
    run_steps(a.warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(a.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dt = dev_all_reduce(t, dist.ReduceOp.MAX).item()
    final_tail = eng.grads[eng.P:].cpu().numpy().astype(np.float64)
    if a.dump_outputs and rank == 0:
        # what a caller of the step receives: the updated parameters and Adam moments, and the last step's [TAIL] loss sums
        dump_outputs(a.dump_outputs, {"params": eng.params.detach().cpu().numpy(), "adam_m": eng.m.cpu().numpy(),
                                      "adam_v": eng.v.cpu().numpy(), "loss_terms": final_tail})
    unit = G if multi_fn is not None else 1
    value = n_gpus * B * d.S * a.steps / dt
    from gmvae_amd import _lib as LIB
    schedule = LIB.step_schedule(eng.dims(B), eng.model)
    line = {
        "metric": "ELBO-samples/sec", "value": value, "unit": "samples/sec", "n_gpus": n_gpus, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3,
        "steps_per_graph_launch": unit, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": PLANES_DTYPE if schedule.endswith("+planes") else "f32", "data": "synthetic",
        "config": {"workload": f"{a.model} train step (noise+fwd+bwd+allreduce+TF-Adam), D={d.D} K={d.K} "
                               f"L={d.L} hidden={hidden} S={d.S}, batch {B}/GPU x {n_gpus} GPU "
                               f"({workload_name(a, n_gpus)})",
                   "global_batch": B * n_gpus, "parallelism": f"dp{n_gpus}", "hipgraph": use_graph, "input_pipeline_on_device": bool(a.pipeline and world == 1), "safe_schedule": safe_schedule,
                   "all_reduce": getattr(eng, "dp_mode", None) if use_graph or world == 1 else "torch.distributed (eager)",
                   "dist_backend": backend if world > 1 else None, "replicas_identical": None},
        "fallback": bool(fallbacks), "fallback_reasons": fallbacks or None,
        "final_loss": final_tail[0] / max(final_tail[4], 1.0),
    }

    def finish(out):
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.destroy_process_group()
        if fallbacks and not a.allow_fallback:
            # the line above carries the slower path's number, marked; the exit code says it is not the path asked for
            raise SystemExit(3)

    if not a.full:
        return finish(line)
    # ---- a short timed region (the driver runs --steps 20: ONE graph launch, 0.8 ms, a single host-clock sample) is
    # repeated: >= 10 more regions of the same K steps, each bracketed like the contract's; median alongside `value`
    region_ms = []
    if dt < 0.05:
        for _ in range(10 if world > 1 else 20):            # (a fixed count: every rank must issue the same collectives)
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            run_steps(a.steps)
            torch.cuda.synchronize()
            region_ms.append((time.perf_counter() - t1) * 1e3 / a.steps)
        region_ms.sort()
    # ---- the same loop once more with HIP events around every graph launch (median, events on the compute
    # stream).  `value` above stays the whole-region host clock the contract prescribes; this is the per-launch view.
    launch_fn = multi_fn if multi_fn is not None else step_fn
    n_ev = int(max(8, min(200, a.steps // unit)))
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_ev)]
    for e0, e1 in evs:
        e0.record()
        launch_fn()
        e1.record()
    torch.cuda.synchronize()
    ev_ms = sorted(e0.elapsed_time(e1) / unit for e0, e1 in evs)
    ms_median_events = ev_ms[len(ev_ms) // 2]
    if world > 1:
        dist.barrier()
    replicas_identical = None
    if world > 1:                                   # every rank must hold bit-identical parameters
        cs = eng.params.detach().double().sum().reshape(1)
        lo, hi = dev_all_reduce(cs.clone(), dist.ReduceOp.MIN), dev_all_reduce(cs.clone(), dist.ReduceOp.MAX)
        replicas_identical = bool((lo == hi).item())
    # the data-parallel step's timeline (device wall clock inside the launches on both sides of the RCCL node; COLLECTIVE:
    # every rank replays the same three-step graph 10 times)
    dp_tl = None
    if dp and use_graph and getattr(eng, "dp_mode", None) == "rccl-in-hipgraph":
        try:
            dp_tl = eng.profile_dp_step(x, lr=1e-3, iters=10)
        except Exception as e:
            dp_tl = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        t_step_us = dt / a.steps * 1e6
        # ---- roofline of the dominant kernel, timed live.  Single device, fused schedules: per launch of the
        # steady-state step (a) its share of the step's TIMELINE -- first workgroup start of the launch to first workgroup
        # start of the next one, device wall clock stamped inside the kernels of a replayed hipGraph: dispatch and
        # end-of-kernel write-back included, the interval rocprofv3 --kernel-trace reports, and the shares add up to the
        # step -- and (b) the in-kernel span (last workgroup end - first workgroup start).  `achieved` / `frac` use (a),
        # so that the committed rocprofv3 average of the same kernel (profiles/) must agree with it.  Other schedules /
        # N > 1: hipEvents around eager launches.
        levels = None
        if dp_tl and "error" not in dp_tl:
            # the DP step's launches with their shares of its timeline (they add up to the step): gradient launch(es), the
            # all-reduce window (RCCL node + the launch boundaries around it), the Adam launch up to the next step's start
            fl_step = flops_per_step(a.model, d.D, d.L, d.K, hidden, d.S, B)
            gname = "+".join(dp_tl["grad_launches"]) or "gradients"
            levels = [(gname, dp_tl["grad_span"], fl_step, dp_tl["grad_span"]),
                      ("rccl_all_reduce", dp_tl["allreduce_window"], 0.0, dp_tl["allreduce_window"]),
                      ("adam_tf_img", dp_tl["adam_span"], 0.0, dp_tl["adam_span"] + dp_tl["gap_to_next_step"])]
        if levels is None and world == 1:
            try:
                levels = eng.profile_train_levels(x, lr=1e-3, iters=30)
            except Exception:
                levels = None
            if levels is None:                           # the skinny schedule stamps the device clock in its own buffer
                try:
                    sk = eng.profile_skinny_levels(x)
                except Exception:
                    sk = None
                if sk:
                    fl = {n: f for n, _, f in eng.profile_levels(x, iters=2)}
                    fl["sk_dw_adam"] = fl.get("sk_dw", 0.0)
                    known = sum(l[3] for l in sk[:-1])
                    levels = [(n, sp, fl.get(n, 0.0), sh if sh is not None else max(t_step_us - known, sp)) for n, sp, _, sh in sk]
        if levels is None:
            levels = eng.profile_levels(x, iters=30)
        levels = [tuple(l) + ((0.0,) if len(l) == 3 else ()) for l in levels]      # (name, span us, flops, timeline us)
        have_tl = all(l[3] > 0 for l in levels)
        dur = (lambda l: l[3]) if have_tl else (lambda l: l[1])
        gemms = [l for l in levels if l[2] > 0]          # launches that do MFMA work (grouped GEMMs, mega kernel)
        dom = max(gemms, key=dur)
        # skinny.hpp: sk_gemm<stage, row tiles per workgroup>; the D-wide layers have a 64-column form (stages 7, 8); the y path a
        # rows-per-workgroup form; the W stage is sk_dw, sk_dwb<.> or sk_dwc
        SK_KERNELS = {"sk_first_layers": ["void gmvae::sk_gemm<0, "], "sk_first_layer": ["void gmvae::sk_gemm<0, "], "sk_q_head_z": ["void gmvae::sk_gemm<1, "],
                      "sk_dec_hidden": ["void gmvae::sk_gemm<2, "], "sk_dec_bernoulli": ["void gmvae::sk_gemm<3, ", "void gmvae::sk_gemm<7, "],
                      "sk_bwd_dhd": ["void gmvae::sk_gemm<4, ", "void gmvae::sk_gemm<8, "], "sk_bwd_dz_heads": ["void gmvae::sk_gemm<5, "],
                      "sk_bwd_dhg": ["void gmvae::sk_gemm<6, "], "sk_y_path": ["void gmvae::sk_ypath<", "void gmvae::sk_ypath_r<"],
                      "sk_y_path_bwd": ["void gmvae::sk_ybwd<", "void gmvae::sk_ybwd_r<"],
                      "sk_gmp_bwd": ["gmvae::sk_gmp_bwd"],
                      "sk_dw_adam": ["gmvae::sk_dw", "void gmvae::sk_dwb<", "gmvae::sk_dwc"],
                      "sk_dw": ["gmvae::sk_dw", "void gmvae::sk_dwb<", "gmvae::sk_dwc"]}
        step_flops = flops_per_step(a.model, d.D, d.L, d.K, hidden, d.S, B)
        # Bytes_alg(step) = B D (uint8 batch) + 9 * 4 P (read params; write grads; Adam reads p, m, v, g and
        # writes p, m, v); noise is generated in-kernel
        step_bytes = float(B * d.D + 36 * eng.P_real)
        t_mfma_us = step_flops / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e6
        t_hbm_us = step_bytes / (PEAK_HBM_GBS * 1e9) * 1e6
        roof = {"bound": "mfma", "kernel": dom[0] if dom[0].startswith(("mega", "sk_", "dw_", "fl_")) else f"gemm_grouped<{dom[0]}>",
                "achieved": dom[2] / dur(dom) * 1e-6, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": dom[2] / dur(dom) * 1e-6 / PEAK_F32_MFMA_TFLOPS,
                "traffic": None, "usec_per_launch": dur(dom), "flops_per_launch": dom[2],
                "usec_in_kernel_span": dom[1], "frac_in_kernel_span": dom[2] / dom[1] * 1e-6 / PEAK_F32_MFMA_TFLOPS,
                "timing": ("launch duration = its share of the step's timeline: first workgroup start -> first workgroup start "
                           "of the next launch (s_memrealtime stamps inside the kernels, steady-state step replayed in a "
                           "hipGraph, mean of 30); usec_in_kernel_span = last workgroup end - first workgroup start")
                          if have_tl else "hipEvents around eager launches",
                # whole step: achieved FLOP/s AND GB/s against the algorithmic counts, and t_step over the
                # larger of the two roofline times
                "step_flops_alg": step_flops, "step_bytes_alg": step_bytes,
                "step_tflops_alg": step_flops / t_step_us * 1e-6, "achieved_gbs": step_bytes / t_step_us * 1e-3,
                "step_frac_of_mfma_peak": step_flops / t_step_us * 1e-6 / PEAK_F32_MFMA_TFLOPS,
                "step_frac_of_hbm_peak": step_bytes / t_step_us * 1e-3 / PEAK_HBM_GBS,
                "t_mfma_usec": t_mfma_us, "t_hbm_usec": t_hbm_us, "t_step_over_ideal": t_step_us / max(t_mfma_us, t_hbm_us),
                # step_flops_executed: what the launches run (S > 1: the layers over the S-times repeated input are
                # computed once per batch row)
                "step_flops_executed": sum(l[2] for l in levels),
                "launches_per_step": len(levels), "sum_launch_usec": sum(dur(l) for l in levels),
                "levels": [[nm, round(us, 2), round(tl, 2)] for nm, us, _, tl in levels],
                "levels_columns": ["launch", "usec_in_kernel_span", "usec_timeline_share"]}
        roof["schedule"] = schedule
        if schedule.endswith("+planes") and dom[0] in ("fwd_dec_bernoulli", "bwd_dec_top"):
            # the launch multiplies fp32 values as piece products on pre-split operands (gemm.hpp plane_rounds2 / plane_rounds3):
            # THREE v_mfma_f32_32x32x16_f16 per product on f16 pairs (SIX ..._bf16 on the exact bf16 triples under
            # GMVAE_PLANES_EXACT=1); its matrix-pipe peak is the dense 16-bit peak / that count in fp32-equivalent FLOP/s
            pk = PEAK_BF16_MFMA_TFLOPS / PLANE_PIECES
            roof.update({"peak": pk, "frac": roof["achieved"] / pk, "frac_in_kernel_span": dom[2] / dom[1] * 1e-6 / pk,
                         "piece_products_per_product": PLANE_PIECES,
                         "peak_note": f"dense f16 / bf16 MFMA peak 2500 TFLOP/s / {PLANE_PIECES:.0f} piece products per fp32 product; fp32 accumulation",
                         "frac_of_f32_mfma_peak": roof["achieved"] / PEAK_F32_MFMA_TFLOPS})
        if dom[0].startswith("sk_dw") and 28.0 * eng.P_real / (PEAK_HBM_GBS * 1e9) >= dom[2] / (PEAK_F32_MFMA_TFLOPS * 1e12):
            # the skinny schedule's longest launch is the weight-gradient + TF-Adam launch: at small batches bound by HBM, not by
            # the matrix pipes -- algorithmic bytes = 7 x 4 P (p, m, v in; p, m, v and the gradient out), SURVEY.md 8(d)'s
            # optimizer term.  (From a few hundred rows its fp32 MFMA time exceeds that: the default "mfma" pricing stands.)
            w_bytes = 28.0 * eng.P_real
            roof.update({"bound": "hbm", "achieved": w_bytes / dur(dom) * 1e-3, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": w_bytes / dur(dom) * 1e-3 / PEAK_HBM_GBS, "bytes_per_launch": w_bytes,
                         "frac_in_kernel_span": w_bytes / dom[1] * 1e-3 / PEAK_HBM_GBS})
        if schedule == "skinny" and B > 128 and roof["bound"] == "mfma":
            # Above 128 rows the skinny schedule's large products run as exact bf16 piece products on the bf16 pipes (skinny.hpp:
            # 3 piece products per product with the uint8 operand, 6 for fp32 x fp32): such a launch is priced against the peak
            # of the instruction it issues -- dense bf16 peak / (piece products per product, FLOP-weighted over the launch's
            # tensors) in fp32-equivalent FLOP/s, as the plane launches above -- with the fp32-MFMA fraction carried beside it.
            h0 = hidden[0]
            pieces = None
            if dom[0] in ("sk_first_layers", "sk_first_layer"):
                pieces, why = 3.0, "the uint8 batch is exact in bf16: 3 piece products per product"
            elif dom[0] in ("sk_dec_bernoulli", "sk_bwd_dhd") and -(-d.D // 64) * -(-B // 16) >= 256:
                pieces, why = 6.0, "fp32 x fp32: 6 piece products per product (64-column form)"
            elif dom[0].startswith("sk_dw"):
                gmv = a.model == "gmvae"
                f_u8 = 2.0 * B * d.D * h0 * (2 if gmv else 1)                     # x^T dY: encoder(_y) and, GMVAE, encoder_gmm's x rows
                f_all = dom[2]
                pieces = (3.0 * f_u8 + 6.0 * max(f_all - f_u8, 0.0)) / max(f_all, 1.0)
                why = (f"FLOP-weighted over the launch's tensors: {f_u8 / f_all:.2f} of its FLOPs with the uint8 operand (3 piece "
                       f"products per product), the rest fp32 x fp32 (6)")
            if pieces:
                pk = PEAK_BF16_MFMA_TFLOPS / pieces
                roof.update({"frac_of_f32_mfma_peak": roof["frac"], "peak": pk, "frac": roof["achieved"] / pk,
                             "frac_in_kernel_span": dom[2] / dom[1] * 1e-6 / pk, "piece_products_per_product": pieces,
                             "peak_note": f"dense bf16 MFMA peak {PEAK_BF16_MFMA_TFLOPS:.0f} TFLOP/s / {pieces:.2f} piece products per "
                                          f"fp32 product ({why}); fp32 accumulation; frac_of_f32_mfma_peak = the same FLOP/s over 157.3"})
            else:
                roof["peak_note"] = "this launch multiplies on the fp32 matrix instruction: fp32 MFMA peak"
        # Committed evidence of the same command (tools/profile_round.sh -> profiles/roundN_*): rocprofv3 --kernel-trace
        # --stats average per kernel, and HBM-side bytes per launch from separate --pmc passes (FETCH_SIZE x2 on gfx950 +
        # WRITE_SIZE; rocprofv3 --pmc cannot run inside this process).  Keyed by workload; the newest round present wins.
        try:
            import csv
            import glob
            tag = {"BASELINE configs[2]": "bench", "per-GPU shard of BASELINE configs[4]": "config5_shard",
                   "bin/run_train.sh sizes": "run_train_sizes", "BASELINE configs[1]": "configs1",
                   "BASELINE configs[0]": "configs0", "BASELINE configs[1] at hidden 512": "configs1_h512",
                   "BASELINE configs[2] at hidden 512": "configs2_h512",
                   "one rank of BASELINE configs[3] on the data-parallel path (one-rank RCCL communicator)": "configs3_dp1",
                   }.get(workload_name(a, n_gpus)) if world == 1 else None
            stats = sorted(glob.glob(os.path.join(ROOT, "profiles", f"round*_{tag}_kernel_stats.csv"))) if tag else []
            kern_us = {}
            if stats:
                for r in csv.DictReader(open(stats[-1])):
                    kern_us[r["Name"]] = float(r["AverageNs"]) * 1e-3
                roof["rocprof_source"] = os.path.relpath(stats[-1], ROOT) + " (rocprofv3 --kernel-trace --stats of this command; a profiled run is slower than the timed one)"
            def is_kernel(k, kn):
                # rocprofv3 names: "gmvae::dw_adam(gmvae::DwArgs)", "void gmvae::mega2_fwd_bwd<0>(gmvae::MegaArgs)", "void gmvae::sk_gemm<1>(...)"
                if not kn:
                    return False
                kn = kn[5:] if kn.startswith("void ") else kn
                k = k[5:] if k.startswith("void ") else k
                return k.startswith(kn) and (kn.endswith((">", "<", ", ")) or k[len(kn):len(kn) + 1] in ("(", "<", " "))
            knames = (["gmvae::mega3_step"] if dom[0].startswith("mega3") else ["gmvae::" + dom[0]]) if dom[0].startswith(("mega", "dw_")) else SK_KERNELS.get(dom[0], [])
            hit = [k for k in kern_us if any(is_kernel(k, kn) for kn in knames)]
            if hit:
                us = sum(kern_us[k] for k in hit)
                roof["rocprof_usec_per_launch"] = us
                roof["rocprof_kernels"] = hit
                roof["frac_rocprof"] = (roof["bytes_per_launch"] / us * 1e-3 / PEAK_HBM_GBS if roof["bound"] == "hbm"
                                        else dom[2] / us * 1e-6 / roof["peak"])
            pl = [k for k in kern_us if k.startswith("void gmvae::gemm_grouped<gmvae::Cfg<128, 128, 32, 2, 2, 1, 2>, 0, %d>" % (2 if PLANES_EXACT else 3))
                  or k.startswith("void gmvae::gemm_grouped<gmvae::Cfg<128, 128, 32, 2, 2, 1, 2>, %d>" % (2 if PLANES_EXACT else 3))]
            px = [k for k in kern_us if k.startswith("void gmvae::gemm_grouped<gmvae::Cfg<256, 128, 32, 4, 2, 1, 2>, 3>")]
            if not hit and px and not PLANES_EXACT and schedule.endswith("+planes") and dom[0] == "bwd_dec_top":
                # f16 pairs: the backward launch (weight + data gradient) runs the 256 x 128 instance, a kernel of its own
                roof["rocprof_usec_per_launch"] = kern_us[px[0]]
                roof["rocprof_kernels"] = px
                roof["frac_rocprof"] = dom[2] / kern_us[px[0]] * 1e-6 / roof["peak"]
            elif not hit and pl and schedule.endswith("+planes") and dom[0] in ("fwd_dec_bernoulli", "bwd_dec_top"):
                # the plane instance runs exactly two launches per step (logits + Bernoulli; weight and data gradient): the
                # committed average is over both, so the fraction is priced on both launches' FLOPs together
                both = [l for l in levels if l[0] in ("fwd_dec_bernoulli", "bwd_dec_top")]
                roof["rocprof_usec_per_launch"] = kern_us[pl[0]]
                roof["rocprof_note"] = "average over the two plane launches of a step (fwd_dec_bernoulli, bwd_dec_top); frac_rocprof = their FLOPs / (2 x average)"
                roof["frac_rocprof"] = sum(l[2] for l in both) / (len(both) * kern_us[pl[0]]) * 1e-6 / roof["peak"]
            traf = sorted(glob.glob(os.path.join(ROOT, "profiles", f"round*_traffic{'' if tag == 'bench' else '_' + str(tag)}.json"))) if tag else []
            if traf:
                tj = json.load(open(traf[-1]))
                roof["traffic_source"] = os.path.relpath(traf[-1], ROOT) + " (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE per launch, separate passes)"
                per = {}
                for nm, _, _, _ in levels:
                    k2 = [k for k in tj if any(is_kernel(k, kn) for kn in SK_KERNELS.get(nm, ["gmvae::mega3_step" if nm.startswith("mega3") else "gmvae::" + nm]))]
                    if k2:
                        per[nm] = sum(tj[k]["hbm_bytes_per_launch"] for k in k2)
                if dom[0] in per:
                    roof["traffic"] = per[dom[0]]
                if len(per) == len(levels):            # every launch of the step is in the PMC record: whole-step traffic
                    roof["traffic_step"] = sum(per.values())
                    roof["traffic_ratio"] = roof["traffic_step"] / step_bytes
                    roof["traffic_per_launch"] = per
                elif a.config == "configs4_shard":
                    # the plane launches by their tile instance: the backward launch (weight + data gradient) runs the 256 x 128
                    # instance on f16 pairs (the 128 x 128 one on bf16 triples), the forward launch (logits + Bernoulli) the 128 x 128
                    # one -- round 5's line took max() over the 128 x 128 entries for both and so reported the FORWARD launch's bytes
                    inst = "Cfg<256, 128" if (dom[0] == "bwd_dec_top" and not PLANES_EXACT) else "Cfg<128, 128"
                    big = [v["hbm_bytes_per_launch"] for k, v in tj.items() if "gemm_grouped<gmvae::" + inst in k]
                    if big and dom[0] in ("bwd_dec_top", "fwd_dec_bernoulli"):
                        roof["traffic"] = max(big)
                        roof["traffic_kernel"] = "gemm_grouped<" + inst + "...> (largest entry of that instance in the PMC record)"
        except Exception as e:
            roof["evidence_error"] = f"{type(e).__name__}: {e}"
        if a.levels:
            for nm, us, fl, tl in levels:
                print(f"  {nm:28s} span {us:9.2f} us  timeline {tl:9.2f} us  {fl / max(dur((nm, us, fl, tl)), 1e-9) * 1e-6:8.2f} TFLOP/s", file=sys.stderr)
        cpu = None
        if not a.no_cpu_baseline:
            r, logical, physical = cpu_baseline(a.model, dims, B, flat0, x_np, eps_np, u_np, a.cpu_seconds)
            best = max(r, key=lambda k: r[k][0])             # the fastest thread count is the baseline
            per_t = ", ".join(f"{k} thread{'s' if k > 1 else ''}: {v[0]:.0f}/s" for k, v in sorted(r.items()))
            cpu = {"value": r[best][0], "unit": "ELBO-samples/sec", "cores": best, "kind": "port",
                   "sample": f"{r[best][1]} full steps (fwd+bwd+TF-Adam, fp32 NumPy/BLAS oracle) of the same B={B} batch on "
                             f"{best} BLAS thread(s), the fastest of [{per_t}] (host: {logical} logical / {physical} physical "
                             f"cores usable; the reference pins intra_op=inter_op=1)",
                   "value_1thread": r[1][0], "value_by_threads": {str(k): v[0] for k, v in sorted(r.items())},
                   "host_logical_cores": logical, "host_physical_cores": physical}
        # the like-for-like number beside the f16-pair plane GEMMs' (<= 3 x 2^-22 per product): the same step on the exact bf16
        # triples (every product exact, GMVAE_PLANES_EXACT=1), re-captured in this process and timed by HIP events
        exact_ms = None
        if world == 1 and use_graph and (roof or {}).get("schedule", "").endswith("+planes") and not PLANES_EXACT:
            try:
                os.environ["GMVAE_PLANES_EXACT"] = "1"
                eng.drop_graphs()
                sxe, rpe = eng.capture_train_step(B, lr=1e-3, n_steps=1)
                sxe.copy_(x)
                for _ in range(5):
                    rpe()
                torch.cuda.synchronize()
                ee = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
                for e0, e1 in ee:
                    e0.record(); rpe(); e1.record()
                torch.cuda.synchronize()
                exact_ms = sorted(e0.elapsed_time(e1) for e0, e1 in ee)[10]
            except Exception as e:
                exact_ms = f"{type(e).__name__}: {e}"
            finally:
                del os.environ["GMVAE_PLANES_EXACT"]
                eng.drop_graphs()
        line["config"]["replicas_identical"] = replicas_identical
        line.update({
            "ms_per_step_median_hip_events": ms_median_events,
            "ms_per_step_median_of_repeats": region_ms[len(region_ms) // 2] if region_ms else None,
            "ms_per_step_repeats": [round(v, 5) for v in region_ms] if region_ms else None,
            "ms_per_step_exact_triples": exact_ms,
            "dp_timeline_usec": dp_tl, "allreduce_usec": (dp_tl or {}).get("allreduce_window"), "rccl_nranks": getattr(eng, "rccl_nranks", None) if dp else None,
            "roofline": roof, "cpu_baseline": cpu, "parity": parity,
        })
    finish(line)


if __name__ == "__main__":
    main()
