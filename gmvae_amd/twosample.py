"""The kernel two-sample test on the device (Gretton et al. 2012): the unbiased MMD^2 between two samples under an rbf kernel (a
mixture of bandwidths) or the energy-distance kernel -|x - y|, its null distribution by permuting the pooled sample, a p-value and
the leave-one-out witness function (include/gmvae_hip.h gmvae_mmd; csrc/twosample.hpp).  Model independent: the samples are any
fp32 [n, D] and [m, D] device tensors -- binary pixels, counts, real features or latent codes.  The statement is
tests/twosample_ref.py."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L

MAX_N, MAX_D, MAX_P, MAX_Q = 1 << 20, 4096, 4096, 8      # the library's gate (include/gmvae_hip.h)
KERNELS = {"rbf": 0, "energy": 1}                        # GMVAE_MMD_RBF, GMVAE_MMD_ENERGY
MEDIAN_ROWS = 1024                                       # bandwidth="median": about this many pooled rows
TOL = 1e-8                                               # a split counts as >= the observed one from mmd2[0] - TOL * kscale on


def check_sizes(N, D, P, Q=1):
    if not (2 <= N <= MAX_N and 1 <= D <= MAX_D):
        raise ValueError(f"the pooled sample must be [N, D] with 2 <= N <= 2^20 and 1 <= D <= {MAX_D}: got [{N}, {D}]")
    if not 1 <= P <= MAX_P:
        raise ValueError(f"the splits (the observed one and the permutations) must number 1 .. {MAX_P}: got {P}")
    if not 1 <= Q <= MAX_Q:
        raise ValueError(f"the rbf kernel takes 1 .. {MAX_Q} bandwidths: got {Q}")


def workspace_bytes(N, D, P):
    b = C.c_uint64()
    L.check(L.lib.gmvae_mmd_workspace_bytes(int(N), int(D), int(P), C.byref(b)), "gmvae_mmd_workspace_bytes")
    return b.value


def _rows(x, what):
    x = torch.as_tensor(x).to(L.require_gpu(), torch.float32)
    x = x.reshape(x.shape[0], -1).contiguous() if x.dim() >= 2 else x
    if x.dim() != 2:
        raise ValueError(f"{what} must be [rows, D]")
    return x


def rms_distance(z):
    """The root-mean-square distance over the pairs i != j of the rows of z [N, D], in closed form: sqrt(2 N / (N - 1) sum_d var_d)
    (fp64 on the device; a 0-d tensor)."""
    N = z.shape[0]
    return (z.double().var(dim=0, unbiased=False).sum() * (2.0 * N / (N - 1))).sqrt()


def median_distance(z):
    """The lower median of the distances over the pairs i < j among the rows arange(0, N, ceil(N / 1024)) of z (fp64 on the
    device; a 0-d tensor)."""
    N = z.shape[0]
    sub = z[torch.arange(0, N, -(-N // MEDIAN_ROWS), device=z.device)].double()
    return torch.pdist(sub).median()


def permutations(n, m, P, seed=0):
    """The splits [P, n + m] (uint8, on the host): row 0 the observed one -- the first n points --, every other row a seeded
    randperm's first n points."""
    N = n + m
    g = torch.Generator().manual_seed(int(seed))
    E = torch.zeros(P, N, dtype=torch.uint8)
    E[0, :n] = 1
    for p in range(1, P):
        E[p, torch.randperm(N, generator=g)[:n]] = 1
    return E


def mmd(z, assignments, kernel="rbf", gamma=(1.0,), rows=True):
    """gmvae_mmd on the pooled sample z [N, D] and the splits [P, N] (non-zero = first sample): (mmd2 [P], row_all [N], row_first
    [N]) in fp64, the two row outputs None with rows=False.  Two launches (energy) or five (rbf) on the current stream; nothing
    synchronises."""
    z = _rows(z, "z")
    N, D = z.shape
    dev = z.device
    E = torch.as_tensor(assignments)
    if E.dim() != 2 or E.shape[1] != N:
        raise ValueError(f"assignments must be [P, N] = [P, {N}]: got {tuple(E.shape)}")
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be one of {sorted(KERNELS)}: got {kernel!r}")
    gamma = [float(g) for g in gamma]      # (the energy kernel takes none: the library ignores gamma and Q there)
    P = E.shape[0]
    check_sizes(N, D, P, len(gamma) if kernel == "rbf" else 1)
    if kernel == "rbf" and any(not (math.isfinite(g) and g >= 0) for g in gamma):
        raise ValueError(f"gamma must be finite and >= 0: got {gamma}")
    E = (E != 0).to(dev, torch.uint8).contiguous() if E.dtype != torch.uint8 else E.to(dev).contiguous()
    out = torch.empty(P, dtype=torch.float64, device=dev)
    row_all = torch.empty(N, dtype=torch.float64, device=dev) if rows else None
    row_first = torch.empty(N, dtype=torch.float64, device=dev) if rows else None
    ws = torch.empty(workspace_bytes(N, D, P), dtype=torch.uint8, device=dev)
    garr = (C.c_double * max(1, len(gamma)))(*gamma)
    L.check(L.lib.gmvae_mmd(L.ptr(z), N, D, L.ptr(E), P, KERNELS[kernel], garr, len(gamma), L.ptr(out), L.ptr(row_all),
                            L.ptr(row_first), L.ptr(ws), L.current_stream()), "gmvae_mmd")
    return out, row_all, row_first


def _gammas(z, kernel, bandwidth, scales):
    """(gamma [Q], sigma) of the rbf kernel: gamma_q = 1 / (2 (scale_q sigma)^2).  gmvae_mmd reads gamma on the host, so a
    bandwidth found on the device ("median", "mean") is read back here: one number."""
    if kernel != "rbf":
        return [], None
    if isinstance(bandwidth, str):
        if bandwidth not in ("median", "mean"):
            raise ValueError(f"bandwidth must be a number, a sequence of numbers, 'median' or 'mean': got {bandwidth!r}")
        sigma = (median_distance(z) if bandwidth == "median" else rms_distance(z)).item()
    elif isinstance(bandwidth, (int, float)):
        sigma = float(bandwidth)
    else:
        sig = [float(s) for s in bandwidth]      # a sequence: the bandwidths themselves, `scales` not applied
        if not sig or any(not (math.isfinite(s) and s > 0) for s in sig):
            raise ValueError(f"every bandwidth must be finite and > 0: got {sig}")
        return [1.0 / (2.0 * s * s) for s in sig], sig
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"the bandwidth must be finite and > 0: got {sigma} (bandwidth={bandwidth!r}; are all rows equal?)")
    scales = [float(s) for s in scales]
    if not scales or any(not (math.isfinite(s) and s > 0) for s in scales):
        raise ValueError(f"every scale must be finite and > 0: got {scales}")
    return [1.0 / (2.0 * (s * sigma) ** 2) for s in scales], sigma


def mmd_test(x, y, n_perms=1000, kernel="rbf", bandwidth="median", scales=(0.5, 1.0, 2.0), seed=0, assignments=None):
    """The two-sample test of x [n, D] against y [m, D].  P = n_perms splits of the pooled sample (x's rows, then y's) in all: split 0
    the observed one, the others `permutations(n, m, P, seed)`; assignments [P, n + m] (non-zero = first sample) replaces them, its
    row 0 then being the split that is tested.  kernel "rbf": k = mean_q exp(-d^2 / (2 (scale_q sigma)^2)), sigma = bandwidth -- a
    number; "median" (median_distance of the pooled rows); "mean" (rms_distance); or a sequence of bandwidths used as they are --;
    "energy": k = -d, MMD^2 the energy distance, bandwidth and scales unused.  A dict of
      mmd2 (0-d fp64): the unbiased MMD^2 of split 0;  null [P - 1]: that of the other splits;
      p_value (0-d fp64) = (1 + #{p >= 1: null[p] >= mmd2 - tol}) / P with tol = 1e-8 kscale, kscale = 1 for rbf and rms_distance
        for energy: a split equal to the observed one (or, at n = m, its complement) counts, as the test's validity requires;
      witness_x [n], witness_y [m]: at each point the mean k to split 0's first sample minus the mean k to its second, the
        point itself left out -- positive where the first sample is denser;
      sigma, n_perms (= P), kscale.
    Where split 0 has fewer than two points on a side, mmd2 is NaN and so are p_value and the witness function.
    bandwidth="median" and "mean" SYNCHRONISE WITH THE HOST: the library reads gamma on the host, so the bandwidth found on the
    device is read back (one .item()).  With a number or a sequence nothing is read back and everything stays on the device."""
    x, y = _rows(x, "x"), _rows(y, "y")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x and y must share D: got {tuple(x.shape)} and {tuple(y.shape)}")
    n, m = x.shape[0], y.shape[0]
    z = torch.cat([x, y])
    N, D = z.shape
    if kernel not in KERNELS:
        raise ValueError(f"kernel must be one of {sorted(KERNELS)}: got {kernel!r}")
    if assignments is None:
        P = int(n_perms)
        check_sizes(N, D, P, 1)
        if n < 1 or m < 1:
            raise ValueError("both samples need at least one row")
        assignments = permutations(n, m, P, seed)
    P = int(torch.as_tensor(assignments).shape[0])
    gamma, sigma = _gammas(z, kernel, bandwidth, scales)
    check_sizes(N, D, P, max(1, len(gamma)))
    out, row_all, row_first = mmd(z, assignments, kernel, gamma)
    kscale = rms_distance(z) if kernel == "energy" else torch.ones((), dtype=torch.float64, device=z.device)
    null = out[1:]
    p_value = (1.0 + (null >= out[0] - TOL * kscale).sum().double()) / P
    p_value = torch.where(torch.isnan(out[0]), out[0], p_value)      # no statistic (a side of split 0 under two points): no p-value
    e0 = (torch.as_tensor(assignments)[0] != 0).to(z.device, torch.float64)
    n0 = e0.sum()
    witness = row_first / (n0 - e0) - (row_all - row_first) / ((N - n0) - (1.0 - e0))
    witness = torch.where(torch.isnan(out[0]), out[0], witness)      # (and no witness function: its leave-one-out means divide by 0)
    return {"mmd2": out[0], "p_value": p_value, "null": null, "witness_x": witness[:n], "witness_y": witness[n:], "sigma": sigma,
            "n_perms": P, "kscale": kscale}


def mmd2(x, y, kernel="rbf", bandwidth="median", scales=(0.5, 1.0, 2.0)):
    """mmd_test without permutations (P = 1): p_value is 1 and null is empty."""
    return mmd_test(x, y, n_perms=1, kernel=kernel, bandwidth=bandwidth, scales=scales)


SPACES = ("data", "code", "both")


PRIOR_SALT = 0x5A17      # the prior draws' seed is model.random_seed * 7919 + PRIOR_SALT


def _prior_draws(model, n):
    """n draws of z from the model's prior where simulate is not available (a likelihood other than the Bernoulli).  Every
    Distribution.sample(seed=s) starts a fresh generator at s, so model.generate_samples -- seeded, like the posterior draw, with
    model.random_seed -- would consume the very normal numbers the posterior draw consumed: the two samples would be paired, the
    pooled sample not exchangeable, the p-value invalid.  The prior is therefore drawn from a stream of its own: a seed derived
    from random_seed, or torch's global generators where the model has none."""
    seed = None if model.random_seed is None else int(model.random_seed) * 7919 + PRIOR_SALT
    if hasattr(model, "encoder_y"):      # the GMVAE: y uniform, then p(z | y)
        K = int(model.mix_components)
        g = None if seed is None else torch.Generator().manual_seed(seed)
        dev = model._need_engine().device
        y = torch.nn.functional.one_hot(torch.randint(0, K, (n,), generator=g).to(dev), K).float()
        return model.prior_gmm(y).sample(seed=seed).reshape(n, -1)
    return model.prior().sample(n, seed=seed).reshape(n, -1)


def model_test(model, images, n_generations=None, space="data", **kw):
    """model.sample_test: the model's samples against `images`, per space a dict of mmd_test(**kw):
      "data": model.simulate(n_generations)["x"] against the binarised images, both as 0 / 1 floats (Bernoulli likelihood only:
        simulate's gate, and its error otherwise);
      "code": one draw of q(z | x) per image against n_generations draws of the prior (simulate's z*) -- whether the aggregate
        posterior matches the prior, with a p-value, next to latent_diagnostics' KL.  The GMVAE's draw is transform's; the VAE's
        and the mixture-prior VAE's is encoder(x).sample(), not the mean transform returns.  Under a likelihood simulate
        refuses, the prior draws come from the prior's own distribution on a stream independent of the posterior draw
        (_prior_draws).
    Not with pixel_mask=True.  n_generations defaults to the number of images.  {"data": ..., "code": ...} with the spaces asked for ("both": both)."""
    return {s: mmd_test(first, second, **kw) for s, (first, second) in model_samples(model, images, n_generations, space).items()}


def model_samples(model, images, n_generations=None, space="data", what="sample_test"):
    """The pairs of samples model.sample_test and model.sample_distance compare, {"data": (simulated x, binarised images), "code":
    (prior draws, posterior draws)} with the spaces asked for, as model_test describes them; `what` names the caller in the
    refusals."""
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}: got {space!r}")
    B = images.shape[0]
    n = B if n_generations is None else int(n_generations)
    eng = model._need_engine()
    if eng.pixel_mask:
        raise ValueError(f"{what} is not available with pixel_mask=True (simulate draws every pixel, and the encoders here "
                         "take no mask)")
    out = {}
    sim = None
    if space in ("data", "both") or eng.likelihood == "bernoulli":
        sim = model.simulate(n)
    if space in ("data", "both"):
        x = torch.as_tensor(images).to(eng.device).reshape(B, -1)
        out["data"] = (sim["x"].float(), (x != 0).float())
    if space in ("code", "both"):
        if hasattr(model, "encoder_y"):
            code = model.transform(images)
        else:
            code = model.encoder(images).sample(seed=model.random_seed)
        prior = sim["z"] if sim is not None else _prior_draws(model, n)
        out["code"] = (prior, code.reshape(B, -1))
    return out
