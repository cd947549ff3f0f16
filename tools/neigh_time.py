"""Time of gmvae_amd.neighbours (include/gmvae_hip.h gmvae_knn_*: exact k-NN, ranks and class sums on the device) at N codes of L
dimensions -- knn, ranks, class_sums and the three scores (leave-one-out k-NN accuracy, silhouette, trustworthiness) -- against a
chunked torch implementation of the same statement on the same device: fp64 differences in [block, N, L] pieces (block sized to
1 GiB), rounded to fp32, then topk / a count of the keys in front / a one-hot fp64 matrix product per class.  The torch side runs the first
`torch_rows` queries against all N references and its time is scaled by N / torch_rows (it is linear in the queries); the line
says so.  One process; device events after a warm-up; every step runs under a time limit of its own (the host polls the step's
closing event; past the limit it prints the line so far and exits with status 3).
    python tools/neigh_time.py [N] [L] [rounds] [torch_rows] [step_limit_s]
(default N = 10,000, L = 64, 3 rounds, 2,048 torch rows, 120 s).  k = 10, C = 10.  Prints one JSON line."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gmvae_amd import neighbours as nb

a = sys.argv[1:]
N, Lz, rounds, trows, limit = (int(v) for v in (a[:5] + ["10000", "64", "3", "2048", "120"][len(a[:5]):]))
K, C_ = 10, 10
FP64_VECTOR_FLOPS = 78.6e12      # the MI355X's fp64 vector peak (public specification)
trows = min(trows, N)
rng = np.random.default_rng(0)
centers = rng.normal(0, 3, (C_, Lz))
lab_np = np.arange(N) % C_
codes = torch.from_numpy((centers[lab_np] + rng.normal(0, 1, (N, Lz))).astype(np.float32)).cuda()
labels = torch.from_numpy(lab_np.astype(np.int32)).cuda()
emb = (codes[:, :2] + 0.5 * torch.randn(N, 2, device="cuda", generator=torch.Generator("cuda").manual_seed(1))).contiguous()
BLK = max(1, (1 << 30) // (N * Lz * 8))
out = {"N": N, "L": Lz, "k": K, "C": C_, "rounds": rounds, "torch_rows": trows, "torch_block": BLK,
       "rows_per_chunk": nb.default_rows(N, N), "workspace_bytes": nb.workspace_bytes(nb.default_rows(N, N), N, Lz, K, C_)}


def wait(event):
    """Polls the event; past the step's limit: the line so far, exit 3."""
    deadline = time.time() + limit
    while not event.query():
        if time.time() > deadline:
            out["timeout_in"] = out.get("step")
            print(json.dumps(out), flush=True)
            os._exit(3)
        time.sleep(0.005)


@torch.no_grad()
def torch_d(c, r0, r1):
    """(D fp64, d fp32) of the rows [r0, r1)"""
    D = (c[r0:r1, None, :].double() - c[None, :, :].double()).square().sum(dim=2)
    return D, D.float()


@torch.no_grad()
def torch_knn(c, rows):
    idx = torch.empty(rows, K, dtype=torch.int64, device=c.device)
    for r0 in range(0, rows, BLK):
        r1 = min(r0 + BLK, rows)
        _, d = torch_d(c, r0, r1)
        d[torch.arange(r1 - r0, device=c.device), torch.arange(r0, r1, device=c.device)] = float("inf")
        idx[r0:r1] = d.topk(K, dim=1, largest=False, sorted=True).indices      # (ties: whatever topk does)
    return idx


@torch.no_grad()
def torch_ranks(c, cand, rows):
    out_ = torch.empty(rows, cand.shape[1], dtype=torch.int64, device=c.device)
    j = torch.arange(c.shape[0], device=c.device)
    for r0 in range(0, rows, BLK):
        r1 = min(r0 + BLK, rows)
        _, d = torch_d(c, r0, r1)
        d[torch.arange(r1 - r0, device=c.device), torch.arange(r0, r1, device=c.device)] = float("inf")
        cj = cand[r0:r1].long()
        dc = d.gather(1, cj)
        for t in range(cand.shape[1]):
            front = (d < dc[:, t:t + 1]) | ((d == dc[:, t:t + 1]) & (j[None, :] < cj[:, t:t + 1]))
            out_[r0:r1, t] = front.sum(dim=1)
    return out_


@torch.no_grad()
def torch_class_sums(c, lab, rows):
    S = torch.empty(rows, C_, dtype=torch.float64, device=c.device)
    onehot = torch.nn.functional.one_hot(lab.long(), C_).double()      # [N, C]: the sums per class are one fp64 matrix product
    for r0 in range(0, rows, BLK):
        r1 = min(r0 + BLK, rows)
        D, _ = torch_d(c, r0, r1)
        S[r0:r1] = D.sqrt() @ onehot
    return S


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    wait(t1)
    return t0.elapsed_time(t1)


cand = nb.knn(emb, k=K)["idx"]
fns = {"hip_knn": lambda: nb.knn(codes, k=K),
       "hip_ranks": lambda: nb.ranks(codes, codes, cand, exclude_self=True),
       "hip_class_sums": lambda: nb.class_sums(codes, codes, labels, C_),
       "hip_knn_accuracy_loo": lambda: nb.knn_accuracy_loo(codes, labels, K, C_),
       "hip_silhouette": lambda: nb.silhouette(codes, labels, C_),
       "hip_trustworthiness": lambda: nb.trustworthiness(codes, emb, K)}
if trows > 0:
    fns.update(torch_knn=lambda: torch_knn(codes, trows), torch_ranks=lambda: torch_ranks(codes, cand, trows),
               torch_class_sums=lambda: torch_class_sums(codes, labels, trows))
ms = {k: [] for k in fns}
for r in range(rounds + 1):                              # round 0 is the warm-up: code objects, the caching allocator
    for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
        out["step"] = f"{k} round {r}"
        t = timed(fns[k])
        if r > 0:
            ms[k].append(t)
for k, v in ms.items():
    scale = N / trows if k.startswith("torch_") else 1.0
    out[f"{k}_ms"] = round(float(np.median(v)) * scale, 3)
    out[f"{k}_min_max_ms"] = [round(min(v) * scale, 3), round(max(v) * scale, 3)]
# the distance stage's arithmetic, a subtraction and a fused multiply-add per pair and dimension, as a share of the fp64 vector peak
for k in ("hip_knn", "hip_ranks", "hip_class_sums"):
    out[f"{k}_fp64_share"] = round(3.0 * N * N * Lz / (out[f"{k}_ms"] * 1e-3) / FP64_VECTOR_FLOPS, 4)
if trows > 0:
    for k in ("knn", "ranks", "class_sums"):
        out[f"torch_over_hip_{k}"] = round(out[f"torch_{k}_ms"] / out[f"hip_{k}_ms"], 1)
    out["step"] = "comparison"
    ti = torch_knn(codes, trows)
    hi = nb.knn(codes, k=K)["idx"][:trows].long()
    tr, hr = torch_ranks(codes, cand, trows), nb.ranks(codes, codes, cand, exclude_self=True)[:trows]
    ts, hs = torch_class_sums(codes, labels, trows), nb.class_sums(codes, codes, labels, C_)[:trows]
    done = torch.cuda.Event()
    done.record()
    wait(done)
    out["knn_rows_equal_to_torch"] = float((ti == hi).all(dim=1).double().mean())
    out["ranks_equal_to_torch"] = float((tr == hr).double().mean())
    out["class_sums_max_rel_diff_vs_torch"] = float(((ts - hs).abs() / hs).max())
out.pop("step", None)
out.update(knn_acc_loo=float(nb.knn_accuracy_loo(codes, labels, K, C_)), silhouette=float(nb.silhouette(codes, labels, C_)["score"]),
           trustworthiness=float(nb.trustworthiness(codes, emb, K)), continuity=float(nb.continuity(codes, emb, K)))
print(json.dumps(out), flush=True)
