"""Exact t-SNE on the device (include/gmvae_hip.h gmvae_tsne_*; csrc/tsne.hpp): what the reference's evaluation does to the
latent code with scikit-learn (scripts/utils.py:148-153, TSNE(n_components=2, perplexity=40, n_iter=300)), O(N^2) per iteration
with no tree, memory O(chunk * N).  Model independent: codes are any fp32 [N, L] device tensor."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

D2_CHUNK_BYTES = 256 << 20      # the affinity stage's chunk of distance rows is at most this large unless `rows` says otherwise


def workspace_bytes(N, Lz, rows=1):
    b = C.c_uint64()
    L.check(L.lib.gmvae_tsne_workspace_bytes(int(N), int(Lz), int(rows), C.byref(b)), "gmvae_tsne_workspace_bytes")
    return b.value


def default_rows(N):
    return max(1, min(int(N), D2_CHUNK_BYTES // (4 * int(N))))


def initial_embedding(N, seed=0, device=None):
    """1e-4 * standard normals [N, 2] from the library's Philox stream (gmvae_noise_fill: row n, key `seed`, step 0)."""
    eps = torch.empty(int(N), 2, dtype=torch.float32, device=device or L.require_gpu())
    L.check(L.lib.gmvae_noise_fill(L.ptr(eps), None, int(N), 2, 1, 0, int(seed), 0, None, L.current_stream()), "gmvae_noise_fill")
    return eps.mul_(1e-4)


def affinities(codes, perplexity, rows=None, workspace=None):
    """(beta, logz, entropy), each [N]: the per-point bandwidths at this perplexity, computed `rows` rows at a time."""
    N, Lz = codes.shape
    rows = default_rows(N) if rows is None else int(rows)
    if not 1 <= rows <= N:
        raise ValueError(f"rows must be in [1, {N}]")
    if workspace is None:
        workspace = torch.empty(workspace_bytes(N, Lz, rows), dtype=torch.uint8, device=codes.device)
    beta, logz, entropy = (torch.empty(N, dtype=torch.float32, device=codes.device) for _ in range(3))
    for r0 in range(0, N, rows):
        L.check(L.lib.gmvae_tsne_affinities(L.ptr(codes), N, Lz, float(perplexity), r0, min(rows, N - r0), L.ptr(beta), L.ptr(logz),
                                            L.ptr(entropy), L.ptr(workspace), L.current_stream()), "gmvae_tsne_affinities")
    return beta, logz, entropy


def gradient(codes, beta, logz, y, exaggeration=1.0, workspace=None):
    """(grad [N, 2], stats [4] = Z, sum p ln w, KL, sum p ln p) at the embedding y."""
    N, Lz = codes.shape
    if workspace is None:
        workspace = torch.empty(workspace_bytes(N, Lz), dtype=torch.uint8, device=codes.device)
    grad = torch.empty(N, 2, dtype=torch.float32, device=codes.device)
    stats = torch.empty(4, dtype=torch.float32, device=codes.device)
    L.check(L.lib.gmvae_tsne_gradient(L.ptr(codes), N, Lz, L.ptr(beta), L.ptr(logz), L.ptr(y), float(exaggeration), L.ptr(grad),
                                      L.ptr(stats), L.ptr(workspace), L.current_stream()), "gmvae_tsne_gradient")
    return grad, stats


def embed(codes, perplexity=40.0, n_iter=300, early_exaggeration=12.0, exaggeration_iters=250, learning_rate="auto", seed=0,
          init=None, rows=None):
    """The 2-D embedding of codes [N, L]: a dict of `embedding` [N, 2], `kl` (at the embedding, a 0-d tensor), `kl_history`
    [n_iter] (the KL each iteration started from), `beta` and `entropy` [N].  The defaults are the reference's call under
    scikit-learn's defaults: early exaggeration 12 with momentum 0.5 for the first min(250, n_iter) iterations, then 1 and
    0.8; learning_rate "auto" = max(N / 48, 50); init: 1e-4 * Philox normals keyed by `seed` unless an [N, 2] tensor is given, or
    "pca" (scikit-learn's default since 1.2): the codes' first two principal components, the first scaled to standard deviation
    1e-4 (gmvae_amd.pca.tsne_init).
    Everything stays on the device; nothing synchronises with the host."""
    dev = L.require_gpu()
    codes = torch.as_tensor(codes).to(dev, torch.float32).contiguous()
    if codes.dim() != 2:
        raise ValueError("codes must be [N, L]")
    N, Lz = codes.shape
    if N < 4 or not 1.0 < float(perplexity) < N - 1:
        raise ValueError(f"perplexity must lie in (1, N - 1) and N >= 4: N = {N}, perplexity = {perplexity}")
    n_iter, exaggeration_iters = int(n_iter), min(int(exaggeration_iters), int(n_iter))
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    lr = max(N / 48.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    rows = default_rows(N) if rows is None else int(rows)
    ws = torch.empty(workspace_bytes(N, Lz, rows), dtype=torch.uint8, device=dev)
    beta, logz, entropy = affinities(codes, perplexity, rows, ws)
    if init is None:
        y = initial_embedding(N, seed, dev)
    elif isinstance(init, str):
        if init != "pca":
            raise ValueError(f'init must be None, "pca" or an [N, 2] tensor: got {init!r}')
        from . import pca
        y = pca.tsne_init(codes)
    else:
        y = torch.as_tensor(init).to(dev, torch.float32).contiguous().clone()
        if y.shape != (N, 2):
            raise ValueError(f"init must be [{N}, 2]")
    vel, gains = torch.zeros_like(y), torch.ones_like(y)
    hist = torch.empty(n_iter, dtype=torch.float32, device=dev)
    L.check(L.lib.gmvae_tsne_run(L.ptr(codes), N, Lz, L.ptr(beta), L.ptr(logz), L.ptr(y), L.ptr(vel), L.ptr(gains), n_iter,
                                 exaggeration_iters, float(early_exaggeration), lr, L.ptr(hist) if n_iter else None, L.ptr(ws),
                                 L.current_stream()), "gmvae_tsne_run")
    _, stats = gradient(codes, beta, logz, y, 1.0, ws)
    return {"embedding": y, "kl": stats[2], "kl_history": hist, "beta": beta, "entropy": entropy}
