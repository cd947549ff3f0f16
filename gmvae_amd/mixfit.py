"""A diagonal Gaussian mixture fitted to latent codes by EM on the device (include/gmvae_hip.h gmvae_mixfit_*; csrc/mixfit.hpp):
the "VAE + GMM" baseline of the deep-clustering tables, and the initialiser of a mixture prior from a pretrained encoder's codes
(VaDE).  Model independent: codes are any fp32 [N, L] device tensor.  The statement is tests/mixfit_ref.py.
covariance="full" fits one L x L covariance per component instead (gmvae_mixfit_full_*; csrc/mixfit_full.hpp; the statement is
tests/mixfit_full_ref.py): scikit-learn's GaussianMixture default, for codes whose clusters are not axis-aligned."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, NamedTuple

import torch

from . import _lib as L

MAX_N, MAX_L, MAX_K, MAX_KL = 1 << 24, 4096, 256, 16384      # the library's gate (include/gmvae_hip.h)
MAX_L_FULL, MAX_KLL_FULL = 128, 1 << 20                      # ... and the full-covariance fit's
COVARIANCES = ("diag", "full")


def _check_sizes(N, Lz, K):
    if not (1 <= N <= MAX_N and 1 <= Lz <= MAX_L):
        raise ValueError(f"codes must be [N, L] with 1 <= N <= 2^24 and 1 <= L <= {MAX_L}: got [{N}, {Lz}]")
    if not (1 <= K <= MAX_K and K * Lz <= MAX_KL):
        raise ValueError(f"K must lie in [1, {MAX_K}] with K * L <= {MAX_KL}: K = {K}, L = {Lz}")


def _check_sizes_full(N, Lz, K):
    if not (1 <= N <= MAX_N and 1 <= Lz <= MAX_L_FULL):
        raise ValueError(f"covariance='full': codes must be [N, L] with 1 <= N <= 2^24 and 1 <= L <= {MAX_L_FULL}: got [{N}, {Lz}]")
    if not (1 <= K <= MAX_K and K * Lz * Lz <= MAX_KLL_FULL):
        raise ValueError(f"covariance='full': K must lie in [1, {MAX_K}] with K * L^2 <= 2^20: K = {K}, L = {Lz}")


class _Kind(NamedTuple):
    """A covariance kind: what `_params`, `assign`, `_run`, the workspace's size and `fit` need to know about it."""
    what: str                    # the mixture's name in a message
    third: str                   # the third parameter's name, next to logw [K] and mu [K, L] ...
    third_shape: Callable        # ... and its shape, of (K, L)
    check_sizes: Callable        # the library's gate for this kind, as a ValueError
    entry: str                   # the library's entry points: entry + "_workspace_bytes", "_assign", "_run"
    info: bool                   # whether assign and run take info_out [K] (int32), ahead of the workspace


_DIAG = _Kind("a mixture", "sigma", lambda K, Lz: (K, Lz), _check_sizes, "gmvae_mixfit", False)
_FULL = _Kind("a full-covariance mixture", "cov", lambda K, Lz: (K, Lz, Lz), _check_sizes_full, "gmvae_mixfit_full", True)
_KINDS = {"diag": _DIAG, "full": _FULL}


def _workspace_bytes(kind, N, Lz, K):
    b, name = C.c_uint64(), kind.entry + "_workspace_bytes"
    L.check(getattr(L.lib, name)(int(N), int(Lz), int(K), C.byref(b)), name)
    return b.value


def workspace_bytes(N, Lz, K):
    return _workspace_bytes(_DIAG, N, Lz, K)


def full_workspace_bytes(N, Lz, K):
    return _workspace_bytes(_FULL, N, Lz, K)


def _codes(codes):
    codes = torch.as_tensor(codes).to(L.require_gpu(), torch.float32).contiguous()
    if codes.dim() != 2:
        raise ValueError("codes must be [N, L]")
    return codes


def is_full(params):
    """Whether `params` is a full-covariance mixture: a dict with `cov`, or a tuple whose third member is 3-D."""
    if isinstance(params, dict):
        return "cov" in params
    return len(params) == 3 and torch.as_tensor(params[2]).dim() == 3


def _params(kind, params, Lz, dev, K=None):
    """(logw [K], mu [K, L], sigma [K, L] or cov [K, L, L]) as fresh contiguous fp32 device tensors, from a tuple or a dict with those keys."""
    if isinstance(params, dict):
        params = (params["logw"], params["mu"], params[kind.third])
    if len(params) != 3:
        raise ValueError(f"{kind.what} is (logw, mu, {kind.third})")
    logw, mu, third = (torch.as_tensor(t).to(dev, torch.float32).contiguous().clone() for t in params)
    k = logw.shape[0] if logw.dim() == 1 else None
    if k is None or mu.shape != (k, Lz) or third.shape != kind.third_shape(k, Lz) or (K is not None and k != K):
        shape = ", ".join(str(n) for n in kind.third_shape("K", Lz))
        raise ValueError(f"{kind.what} is logw [K], mu [K, {Lz}], {kind.third} [{shape}]"
                         + (f" with K = {K}" if K is not None else "")
                         + f": got {tuple(logw.shape)}, {tuple(mu.shape)}, {tuple(third.shape)}")
    return logw, mu, third


def _info(kind, K, dev):
    """The info_out argument of a kind's assign and run: (the tensor or None, the arguments it adds to the call)."""
    if not kind.info:
        return None, ()
    info = torch.empty(K, dtype=torch.int32, device=dev)
    return info, (L.ptr(info),)


def _assign(kind, codes, params, workspace=None):
    N, Lz = codes.shape
    logw, mu, third = _params(kind, params, Lz, codes.device)
    K = logw.shape[0]
    kind.check_sizes(N, Lz, K)
    if workspace is None:
        workspace = torch.empty(_workspace_bytes(kind, N, Lz, K), dtype=torch.uint8, device=codes.device)
    log_resp = torch.empty(N, K, dtype=torch.float32, device=codes.device)
    lse = torch.empty(N, dtype=torch.float32, device=codes.device)
    info, info_arg = _info(kind, K, codes.device)
    name = kind.entry + "_assign"
    L.check(getattr(L.lib, name)(L.ptr(codes), N, Lz, K, L.ptr(logw), L.ptr(mu), L.ptr(third), L.ptr(log_resp), L.ptr(lse), *info_arg,
                                 L.ptr(workspace), L.current_stream()), name)
    return {"log_resp": log_resp, "lse": lse, **({"info": info} if kind.info else {})}


def assign(codes, params, workspace=None):
    """The E-step of codes [N, L] under the mixture `params` = (logw, mu, sigma) or a dict with those keys (fit's): a dict of
    `log_resp` [N, K] = ln r_nk and `lse` [N] = ln p(z_n).  A dict with `cov`, or a tuple whose third member is 3-D, is a
    full-covariance mixture (logw, mu, cov [K, L, L]): the dict then also holds `info` [K] (int32), the factorisation's verdict on
    each covariance -- 0, or j + 1 for the first pivot j that is not > 0, and that component's column of `log_resp` is -inf."""
    return _assign(_FULL if is_full(params) else _DIAG, _codes(codes), params, workspace)


def uniforms(K, seed=0, device=None):
    """The K uniforms of a seeding: row 0 of gmvae_noise_fill's `u` output, key `seed`, step 0."""
    u = torch.empty(1, int(K), dtype=torch.float32, device=device or L.require_gpu())
    L.check(L.lib.gmvae_noise_fill(None, L.ptr(u), 1, 1, int(K), 0, int(seed), 0, None, L.current_stream()), "gmvae_noise_fill")
    return u[0]


def kmeanspp(codes, K, seed=0):
    """k-means++ seeding: the int64 [K] indices of the chosen rows.  i_0 = min(floor(u_0 N), N - 1); for k >= 1, d2min_n = the
    smallest squared distance (fp64 differences) to the centres so far, c = its fp64 cumulative sum in index order, i_k = the first
    index with c > u_k c[N-1] (c[N-1] = 0: i_k = min(floor(u_k N), N - 1)); u = uniforms(K, seed).  K rounds of a few torch ops on
    the device; nothing synchronises with the host."""
    codes = _codes(codes)
    N, Lz = codes.shape
    K = int(K)
    _check_sizes(N, Lz, K)
    z = codes.double()
    u = uniforms(K, seed, codes.device).double()
    last = torch.tensor(N - 1, dtype=torch.int64, device=codes.device)
    fallback = torch.minimum(torch.floor(u * N).to(torch.int64), last)      # [K]
    idx = [fallback[0]]
    d2 = ((z - z.index_select(0, idx[0].view(1))) ** 2).sum(dim=1)
    for k in range(1, K):
        c = torch.cumsum(d2, dim=0)
        i = torch.minimum(torch.searchsorted(c, (u[k] * c[-1]).view(1), right=True)[0], last)
        i = torch.where(c[-1] == 0, fallback[k], i)
        idx.append(i)
        d2 = torch.minimum(d2, ((z - z.index_select(0, i.view(1))) ** 2).sum(dim=1))
    return torch.stack(idx)


def _run(kind, codes, logw, mu, third, reg_covar, n_iter, ws):
    """n_iter iterations in place; (loglik_history [n_iter], counts [K], info [K] or None).  n_iter = 0: counts = the E-step's R_k
    at the start, and info that E-step's."""
    N, Lz = codes.shape
    K = logw.shape[0]
    hist = torch.empty(n_iter, dtype=torch.float32, device=codes.device)
    counts = torch.empty(K, dtype=torch.float32, device=codes.device)
    info, info_arg = _info(kind, K, codes.device)
    name = kind.entry + "_run"
    L.check(getattr(L.lib, name)(L.ptr(codes), N, Lz, K, L.ptr(logw), L.ptr(mu), L.ptr(third), float(reg_covar), n_iter,
                                 L.ptr(hist) if n_iter else None, L.ptr(counts), *info_arg, L.ptr(ws), L.current_stream()), name)
    if n_iter == 0:
        a = _assign(kind, codes, (logw, mu, third), ws)
        counts, info = a["log_resp"].double().exp().sum(dim=0).float(), a.get("info")
    return hist, counts, info


def fit(codes, K, n_iter=100, n_init=1, reg_covar=1e-6, seed=0, init=None, covariance="diag"):
    """EM for a K-component diagonal Gaussian mixture on codes [N, L]: a dict of `logw` [K], `mu` and `sigma` [K, L], `counts` [K]
    (R_k of the last iteration), `loglik` (1/N sum_n ln p(z_n) at the returned parameters, from one assign pass after the run; a
    0-d fp64 tensor), `loglik_history` [n_iter] (the value each iteration started from) and `centres` (the int64 [K] rows the
    seeding chose).  The start: mu = the rows kmeanspp(codes, K, seed) chose, sigma = every component at the per-dimension standard
    deviation of all codes (fp64, floored at sqrt(reg_covar)), logw = -ln K.  init = (logw, mu, sigma) replaces the seeding;
    `centres` is then None.  n_init > 1 runs the seeds seed, seed + 1, ... and returns the run with the largest final `loglik`
    (init and n_init > 1 exclude each other).  A fixed number of iterations, no stopping rule: the history is returned.
    covariance="full": one covariance per component -- `cov` [K, L, L] (symmetric) in place of `sigma`, and `info` [K] (int32: 0, or
    j + 1 where a factorisation first met a pivot j that was not > 0; such a component sits that E-step out and restarts from
    reg_covar I).  The same seeding and logw; cov_k = diag(sd^2) of all codes floored at reg_covar, so the first E-step is the
    diagonal fit's.  init = (logw, mu, cov [K, L, L]).  L <= 128 and K L^2 <= 2^20.
    Everything stays on the device; nothing synchronises with the host."""
    codes = _codes(codes)
    N, Lz = codes.shape
    K, n_iter, n_init = int(K), int(n_iter), int(n_init)
    if covariance not in COVARIANCES:
        raise ValueError(f"covariance must be one of {COVARIANCES}: got {covariance!r}")
    kind = _KINDS[covariance]
    _check_sizes(N, Lz, K)
    kind.check_sizes(N, Lz, K)
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    if n_init < 1:
        raise ValueError("n_init must be >= 1")
    if not (math.isfinite(float(reg_covar)) and float(reg_covar) > 0):
        raise ValueError("reg_covar must be a finite number > 0")
    if init is not None and n_init != 1:
        raise ValueError("init replaces the seeding: n_init must be 1")
    dev = codes.device
    ws = torch.empty(_workspace_bytes(kind, N, Lz, K), dtype=torch.uint8, device=dev)
    runs = []
    for j in range(n_init):
        if init is not None:
            if kind is _FULL and not is_full(init):
                raise ValueError("covariance='full' takes init = (logw, mu, cov [K, L, L])")
            logw, mu, third = _params(kind, init, Lz, dev, K)
            centres = None
        else:
            centres = kmeanspp(codes, K, int(seed) + j)
            mu = codes.index_select(0, centres).contiguous()
            logw = torch.full((K,), -math.log(K), dtype=torch.float32, device=dev)
            if kind is _FULL:
                var = codes.double().var(dim=0, unbiased=False).clamp_min(float(reg_covar))
                third = torch.diag(var).float().expand(K, Lz, Lz).contiguous()
            else:
                sd = codes.double().std(dim=0, unbiased=False).clamp_min(math.sqrt(float(reg_covar)))
                third = sd.float().expand(K, Lz).contiguous()
        hist, counts, info = _run(kind, codes, logw, mu, third, reg_covar, n_iter, ws)
        loglik = _assign(kind, codes, (logw, mu, third), ws)["lse"].double().mean()
        runs.append({"logw": logw, "mu": mu, kind.third: third, "counts": counts, "loglik": loglik, "loglik_history": hist,
                     "centres": centres, **({"info": info} if kind.info else {})})
    if n_init == 1:
        return runs[0]
    best = torch.stack([r["loglik"] for r in runs]).argmax().view(1)      # (a NaN loglik would win the argmax: it is then reported)
    return {k: torch.stack([r[k] for r in runs]).index_select(0, best)[0] for k in runs[0]}


def n_parameters(K, Lz, covariance="diag"):
    """The free parameters of a K-component mixture in L dimensions (scikit-learn's GaussianMixture._n_parameters): K - 1 weights,
    K L means, and K L variances (diag) or K L (L + 1) / 2 covariance entries (full)."""
    if covariance not in COVARIANCES:
        raise ValueError(f"covariance must be one of {COVARIANCES}: got {covariance!r}")
    K, Lz = int(K), int(Lz)
    return K - 1 + K * Lz + (K * Lz * (Lz + 1) // 2 if covariance == "full" else K * Lz)


def _fit_parameters(fit_dict):
    K, Lz = fit_dict["mu"].shape
    return n_parameters(K, Lz, "full" if "cov" in fit_dict else "diag")


def bic(fit_dict, N):
    """The Bayesian information criterion of a fit (either covariance) on the N codes it was fitted to: -2 N loglik + p ln N
    (scikit-learn's definition; smaller is better).  A 0-d fp64 tensor; nothing synchronises with the host."""
    return -2.0 * int(N) * fit_dict["loglik"].double() + _fit_parameters(fit_dict) * math.log(int(N))


def aic(fit_dict, N):
    """The Akaike information criterion: -2 N loglik + 2 p."""
    return -2.0 * int(N) * fit_dict["loglik"].double() + 2.0 * _fit_parameters(fit_dict)


def softplus_inverse(sigma):
    """raw with softplus(raw) = sigma: sigma + ln(-expm1(-sigma)), evaluated in fp64, returned in fp32."""
    s = sigma.double()
    return (s + torch.log(-torch.expm1(-s))).float()


def fit_latent(model, images, n_components, **kw):
    """model.fit_latent_mixture: fit(model.transform(images), n_components, **kw) plus `log_resp` [N, K] of those codes."""
    if n_components is None:
        raise ValueError("n_components is required: this model has no mixture to take the number of components from")
    codes = _codes(model.transform(images))
    out = fit(codes, int(n_components), **kw)
    out["log_resp"] = assign(codes, out)["log_resp"]
    return out


def checked_fit(fit_dict, K, Lz, dev):
    """(logw, mu, sigma) of a fit for a prior of K components in L dimensions, or ValueError."""
    if is_full(fit_dict):
        raise ValueError("the fitted mixture has full covariances and this model's priors are diagonal: fit with covariance='diag'")
    try:
        return _params(_DIAG, fit_dict, Lz, dev, K)
    except ValueError as e:
        raise ValueError(f"the fitted mixture does not match this model's prior (K = {K}, L = {Lz}): {e}") from None
