"""The debiased Sinkhorn divergence between two samples on the device (Genevay et al. 2018; Feydy et al. 2019): a transport distance
under the cost 1/2 |u - v|^2, in the data's own units -- 1/2 squared distance per unit of mass moved --, its per-point contributions,
a convergence readout and a permutation null (include/gmvae_hip.h gmvae_sinkhorn; csrc/sinkhorn.hpp).  Model independent: the samples
are any fp32 [n, D] and [m, D] device tensors -- binary pixels, counts, real features or latent codes.  The statement is
tests/sinkhorn_ref.py.

What the number is and is not (profiles/sinkhorn_notes.md):
  * CONVERGENCE DEPENDS ON THE DATA.  `marginal_err` -- the relative error of the transport plan's row marginals -- is always
    returned: at the defaults it is 2e-3 on Gaussian codes, 2e-7 on pixel-like data after 50 iterations, but 3e-2 .. 6e-2 on ten
    well-separated clusters, where the divergence is still 0.4 .. 3 % below its converged value.  Raise n_iter or blur_rel until it
    is small.
  * FINITE-SAMPLE BIAS.  Two samples of one distribution do not give 0: at n = 300 about 0.05 .. 0.07 cscale.  The divergence has
    no zero point at finite n; divergence_test gives it one by permutation.
  * It compares like with like only at equal n, m and blur."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from . import twosample

MAX_N, MAX_D, MAX_ITER = 1 << 20, 4096, 100000      # the library's gate (include/gmvae_hip.h)
TOL = 1e-8                                           # a split counts as >= the observed one from S - TOL * cscale on


def check_sizes(n, m, D, n_iter=1):
    if not (1 <= n <= MAX_N and 1 <= m <= MAX_N and 1 <= D <= MAX_D):
        raise ValueError(f"the samples must be [n, D] and [m, D] with 1 <= n, m <= 2^20 and 1 <= D <= {MAX_D}: got [{n}, {D}] and [{m}, {D}]")
    if not 1 <= n_iter <= MAX_ITER:
        raise ValueError(f"n_iter must lie in [1, {MAX_ITER}]: got {n_iter}")


def workspace_bytes(n, m, D):
    b = C.c_uint64()
    L.check(L.lib.gmvae_sinkhorn_workspace_bytes(int(n), int(m), int(D), C.byref(b)), "gmvae_sinkhorn_workspace_bytes")
    return b.value


def _check_blur(blur, blur_rel):
    """A blur (or blur_rel) given as a number must be finite and > 0; a tensor is taken as it is (nothing is read back)."""
    for name, v in (("blur", blur), ("blur_rel", blur_rel)):
        if isinstance(v, (int, float)) and not (math.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be finite and > 0: got {v}")


def _check_iters(n_iter, n_final):
    n_iter = int(n_iter)
    if not 1 <= n_iter <= MAX_ITER:
        raise ValueError(f"n_iter must lie in [1, {MAX_ITER}]: got {n_iter}")
    n_final = n_iter // 4 if n_final is None else int(n_final)
    if not 0 <= n_final <= n_iter:
        raise ValueError(f"n_final must lie in [0, n_iter]: got {n_final}")
    return n_iter, n_final


def schedule(z_pooled, n_iter=200, blur=None, blur_rel=0.1, n_final=None):
    """The temperatures eps [n_iter + 1] (fp64, on z_pooled's device; nothing is read back) for the pooled sample z_pooled [N, D]:
    eps[n_iter] = blur^2 with blur = blur_rel * twosample.rms_distance(z_pooled) unless given; eps[0] = max((2 max_i |z_i - mean|)^2,
    blur^2), the squared diameter of a ball that holds the sample; geometric from eps[0] to blur^2 over the first K = n_iter -
    n_final entries (eps[i] = eps[0] (blur^2 / eps[0])^(i / K)), blur^2 from entry K on.  n_final defaults to n_iter // 4."""
    _check_blur(blur, blur_rel)
    T, n_final = _check_iters(n_iter, n_final)
    z = z_pooled.double()
    if blur is None:
        blur = blur_rel * twosample.rms_distance(z_pooled)
    eT = torch.as_tensor(blur, dtype=torch.float64, device=z.device) ** 2
    r2 = ((z - z.mean(dim=0)) ** 2).sum(dim=1).max()
    e0 = torch.maximum(4.0 * r2, eT)
    K = T - n_final
    i = torch.arange(T + 1, dtype=torch.float64, device=z.device)
    frac = (i / K).clamp(max=1.0) if K > 0 else torch.ones_like(i)
    return torch.where(frac >= 1.0, eT, torch.exp(e0.log() + frac * (eT.log() - e0.log())))


def _rows(x, what):
    return twosample._rows(x, what)


def _weights(w, count, what, dev):
    if w is None:
        return None
    w = torch.as_tensor(w).to(dev, torch.float64).contiguous()
    if w.shape != (count,):
        raise ValueError(f"{what} must be [{count}]: got {tuple(w.shape)}")
    return w


def solve(x, y, eps, a=None, b=None):
    """gmvae_sinkhorn on x [n, D], y [m, D] (fp32), the schedule eps [n_iter + 1] (fp64, on the device) and the weights a [n], b [m]
    (fp64, positive; None: uniform): a dict of sinkhorn, part_x, part_y, marginal_err (0-d fp64), contrib_x [n] = f - p, contrib_y
    [m] = g - q -- positive where a point is far from the other sample: the counterpart of the MMD's witness function --, the
    potentials f, g, p, q and eps.  Enqueued on the current stream; nothing synchronises."""
    x, y = _rows(x, "x"), _rows(y, "y")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x and y must share D: got {tuple(x.shape)} and {tuple(y.shape)}")
    (n, D), m = x.shape, y.shape[0]
    dev = x.device
    eps = torch.as_tensor(eps).to(dev, torch.float64).contiguous()
    if eps.dim() != 1 or eps.shape[0] < 2:
        raise ValueError(f"eps must be [n_iter + 1] with n_iter >= 1: got {tuple(eps.shape)}")
    n_iter = eps.shape[0] - 1
    check_sizes(n, m, D, n_iter)
    a, b = _weights(a, n, "a", dev), _weights(b, m, "b", dev)
    f, p = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    g, q = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(2))
    out = torch.empty(4, dtype=torch.float64, device=dev)
    ws = torch.empty(workspace_bytes(n, m, D), dtype=torch.uint8, device=dev)
    L.check(L.lib.gmvae_sinkhorn(L.ptr(x), n, L.ptr(y), m, D, L.ptr(a), L.ptr(b), L.ptr(eps), n_iter, L.ptr(f), L.ptr(g), L.ptr(p),
                                 L.ptr(q), L.ptr(out), L.ptr(ws), L.current_stream()), "gmvae_sinkhorn")
    return {"sinkhorn": out[0], "part_x": out[1], "part_y": out[2], "marginal_err": out[3], "contrib_x": f - p, "contrib_y": g - q,
            "f": f, "g": g, "p": p, "q": q, "eps": eps}


def _check_pair(x, y, n_iter, n_final, blur, blur_rel):
    """The checks of divergence and divergence_test, before any launch."""
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x and y must share D: got {tuple(x.shape)} and {tuple(y.shape)}")
    n_iter, n_final = _check_iters(n_iter, n_final)
    check_sizes(x.shape[0], y.shape[0], x.shape[1], n_iter)
    _check_blur(blur, blur_rel)
    return n_iter, n_final


def divergence(x, y, blur=None, blur_rel=0.1, n_iter=200, n_final=None, a=None, b=None):
    """The debiased Sinkhorn divergence of x [n, D] against y [m, D] at the temperature blur^2 -- blur in the data's units, by default
    blur_rel times the root-mean-square distance of the pooled sample --, annealed over `schedule(pooled, n_iter, blur, blur_rel,
    n_final)`.  solve's dict plus cscale (0-d fp64) = rms_distance^2 / 2, the mean cost over the pairs of the pooled sample: the
    unit in which the divergence reads as a fraction.  All device tensors; nothing is read back.
    ALWAYS LOOK AT marginal_err: convergence depends on the data (the module's docstring), and the divergence is low until it is
    small.  Two samples of one distribution give a positive value at finite n (divergence_test); values compare only at equal n, m
    and blur.  A sample whose rows are all equal has no blur of its own: give `blur`."""
    x, y = _rows(x, "x"), _rows(y, "y")
    n_iter, n_final = _check_pair(x, y, n_iter, n_final, blur, blur_rel)
    z = torch.cat([x, y])
    out = solve(x, y, schedule(z, n_iter, blur, blur_rel, n_final), a, b)
    out["cscale"] = 0.5 * twosample.rms_distance(z) ** 2
    return out


def divergence_test(x, y, n_perms=100, seed=0, **kw):
    """divergence with a permutation null: P = n_perms splits of the pooled sample (x's rows, then y's) in all, split 0 the observed
    one, the others `twosample.permutations(n, m, P, seed)` -- the MMD test's seeded splits --, one library call a split, the
    schedule built once from the pooled sample and shared.  divergence's dict (of the observed split) plus null [P - 1] and p_value
    = (1 + #{null >= sinkhorn - 1e-8 cscale}) / P, the MMD test's tie rule.  The weights a and b, if given, stay with the positions
    (row i of the first sample has weight a[i] in every split)."""
    x, y = _rows(x, "x"), _rows(y, "y")
    blur, blur_rel = kw.pop("blur", None), kw.pop("blur_rel", 0.1)
    n_iter, n_final = _check_pair(x, y, kw.pop("n_iter", 200), kw.pop("n_final", None), blur, blur_rel)
    a, b = kw.pop("a", None), kw.pop("b", None)
    if kw:
        raise TypeError(f"unexpected arguments: {sorted(kw)}")
    P = int(n_perms)
    if not 1 <= P <= twosample.MAX_P:
        raise ValueError(f"the splits (the observed one and the permutations) must number 1 .. {twosample.MAX_P}: got {P}")
    n, m = x.shape[0], y.shape[0]
    z = torch.cat([x, y])
    eps = schedule(z, n_iter, blur, blur_rel, n_final)
    out = solve(x, y, eps, a, b)
    out["cscale"] = 0.5 * twosample.rms_distance(z) ** 2
    E = twosample.permutations(n, m, P, seed)      # (on the host: the rows of a split are gathered by index, nothing is read back)
    null = torch.empty(P - 1, dtype=torch.float64, device=z.device)
    for s in range(1, P):
        first, second = (E[s] != 0).nonzero().flatten().to(z.device), (E[s] == 0).nonzero().flatten().to(z.device)
        null[s - 1] = solve(z[first], z[second], eps, a, b)["sinkhorn"]
    out["null"] = null
    out["p_value"] = (1.0 + (null >= out["sinkhorn"] - TOL * out["cscale"]).sum().double()) / P
    out["n_perms"] = P
    return out


def model_distance(model, images, n_generations=None, space="data", n_perms=0, **kw):
    """model.sample_distance: the Sinkhorn divergence between the model's samples and `images`, on the pairs of samples
    model.sample_test compares (twosample.model_samples: the same draws, seeds and refusals), per space a dict of divergence(**kw)
    -- or, with n_perms > 0, of divergence_test(n_perms=n_perms, **kw)."""
    out = {}
    for space, (first, second) in twosample.model_samples(model, images, n_generations, space, "sample_distance").items():
        out[space] = divergence_test(first, second, n_perms=n_perms, **kw) if n_perms else divergence(first, second, **kw)
    return out
