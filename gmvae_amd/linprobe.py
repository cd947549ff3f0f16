"""A linear probe on latent codes: multinomial logistic regression with an l2 penalty, fitted on the device by FISTA in the fixed
metric of Boehning's bound (include/gmvae_hip.h gmvae_linprobe_*; csrc/linprobe.hpp) -- the linear-classifier accuracy that
representation papers report next to k-NN accuracy, and with a few labels per class the "M1" baseline of Kingma et al. 2014.  Model
independent: codes are any fp32 [N, L] device tensor.  The statement is tests/linprobe_ref.py."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L

MAX_N, MAX_L, MAX_C, MAX_CL = 1 << 24, 128, 256, 16384      # the library's gate (include/gmvae_hip.h)


def check_sizes(N, Lz, n_classes):
    if not (1 <= N <= MAX_N and 1 <= Lz <= MAX_L):
        raise ValueError(f"codes must be [N, L] with 1 <= N <= 2^24 and 1 <= L <= {MAX_L}: got [{N}, {Lz}]")
    if not (2 <= n_classes <= MAX_C and n_classes * Lz <= MAX_CL):
        raise ValueError(f"n_classes must lie in [2, {MAX_C}] with n_classes * L <= {MAX_CL}: n_classes = {n_classes}, L = {Lz}")


def workspace_bytes(N, Lz, n_classes):
    b = C.c_uint64()
    L.check(L.lib.gmvae_linprobe_workspace_bytes(int(N), int(Lz), int(n_classes), C.byref(b)), "gmvae_linprobe_workspace_bytes")
    return b.value


def _codes(codes):
    codes = torch.as_tensor(codes).to(L.require_gpu(), torch.float32).contiguous()
    if codes.dim() != 2:
        raise ValueError("codes must be [N, L]")
    return codes


def _labels(labels, N, n_classes, dev, need_one):
    """int32 [N] on the device.  Labels that arrive on the host are checked there for one labelled row; labels already on the device
    are not read back -- a fit without a labelled row then reports info = -1."""
    t = torch.as_tensor(labels)
    if t.shape != (N,):
        raise ValueError(f"labels must be [N] = [{N}]: got {tuple(t.shape)}")
    if need_one and not t.is_cuda and not bool(((t >= 0) & (t < n_classes)).any()):
        raise ValueError(f"no label lies in [0, {n_classes}): the fit needs at least one labelled row")
    return t.to(dev, torch.int32).contiguous()


def _standardise(codes, params):
    if isinstance(params, dict) and "mean" in params:
        return ((codes.double() - params["mean"]) / params["scale"]).float().contiguous()
    return codes


def fit(codes, labels, n_classes, l2=1e-3, n_iter=300, standardize=False):
    """Softmax regression of `labels` [N] (an int outside [0, n_classes) -- runners.select_labelled's -1 -- marks the row
    unlabelled: weight 0) on codes [N, L]: minimises -(1/n) sum_labelled ln p_n[y_n] + (l2 / 2) |W|_F^2 over W [L, C] and a free
    bias b [C] by n_iter iterations of FISTA in the metric A = 1/2 Cov_labelled(x) + l2 I (unit steps, no line search, no stopping
    rule).  A dict of `W`, `b` (the logits are codes @ W + b), `loss_history` [n_iter] (the objective at the point each iteration
    evaluated; not monotone -- FISTA is not), `grad_max` (0-d: max |gradient| at the last evaluated point, the convergence readout),
    `info` (0-d int32: 0; j + 1 if A's factorisation met a pivot j that is not > 0, or -1 if no row is labelled -- W and b are then
    0 and the history NaN).  standardize: the codes are first centred and scaled per dimension by the labelled
    rows' mean and standard deviation (torch fp64; a constant dimension keeps scale 1); the dict then holds `mean` and `scale`
    [L], which predict and score apply.  1 <= L <= 128, 2 <= n_classes <= 256, n_classes * L <= 16,384.
    Everything stays on the device; 3 + 2 n_iter launches and nothing synchronises with the host."""
    codes = _codes(codes)
    N, Lz = codes.shape
    n_classes, n_iter, l2 = int(n_classes), int(n_iter), float(l2)
    check_sizes(N, Lz, n_classes)
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    if not (math.isfinite(l2) and l2 > 0):
        raise ValueError("l2 must be a finite number > 0")
    dev = codes.device
    y = _labels(labels, N, n_classes, dev, True)
    extra = {}
    if standardize:
        w = ((y >= 0) & (y < n_classes)).double().unsqueeze(1)
        n = w.sum().clamp_min(1.0)
        x = codes.double()
        mean = (w * x).sum(dim=0) / n
        sd = ((w * (x - mean) ** 2).sum(dim=0) / n).sqrt()
        extra = {"mean": mean, "scale": torch.where(sd > 0, sd, torch.ones_like(sd))}
        codes = _standardise(codes, extra)
    W = torch.empty(Lz, n_classes, dtype=torch.float32, device=dev)
    b = torch.empty(n_classes, dtype=torch.float32, device=dev)
    hist = torch.empty(n_iter, dtype=torch.float32, device=dev)
    grad_max = torch.empty(1, dtype=torch.float32, device=dev)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(N, Lz, n_classes), dtype=torch.uint8, device=dev)
    L.check(L.lib.gmvae_linprobe_fit(L.ptr(codes), L.ptr(y), N, Lz, n_classes, l2, n_iter, L.ptr(W), L.ptr(b),
                                     L.ptr(hist) if n_iter else None, L.ptr(grad_max), L.ptr(info), L.ptr(ws), L.current_stream()),
            "gmvae_linprobe_fit")
    return {"W": W, "b": b, "loss_history": hist, "grad_max": grad_max[0], "info": info[0], **extra}


def _params(params, Lz, dev):
    W, b = (params["W"], params["b"]) if isinstance(params, dict) else params
    W = torch.as_tensor(W).to(dev, torch.float32).contiguous()
    b = torch.as_tensor(b).to(dev, torch.float32).contiguous()
    if W.dim() != 2 or W.shape[0] != Lz or b.shape != (W.shape[1],):
        raise ValueError(f"a probe is W [{Lz}, C] and b [C]: got {tuple(W.shape)} and {tuple(b.shape)}")
    return W, b


def _predict(codes, params, labels):
    codes = _standardise(_codes(codes), params)
    N, Lz = codes.shape
    dev = codes.device
    W, b = _params(params, Lz, dev)
    n_classes = W.shape[1]
    check_sizes(N, Lz, n_classes)
    y = None if labels is None else _labels(labels, N, n_classes, dev, False)
    log_prob = torch.empty(N, n_classes, dtype=torch.float32, device=dev)
    pred = torch.empty(N, dtype=torch.int32, device=dev)
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    ws = torch.empty(workspace_bytes(N, Lz, n_classes), dtype=torch.uint8, device=dev)
    L.check(L.lib.gmvae_linprobe_predict(L.ptr(codes), L.ptr(y), N, Lz, n_classes, L.ptr(W), L.ptr(b), L.ptr(log_prob), L.ptr(pred),
                                         L.ptr(sums), L.ptr(ws), L.current_stream()), "gmvae_linprobe_predict")
    return log_prob, pred, sums


def predict(codes, params):
    """The probe `params` (fit's dict, or (W, b)) on codes [N, L]: a dict of `log_prob` [N, C] = ln softmax(codes @ W + b) and
    `pred` [N] (int32), its first maximal index."""
    log_prob, pred, _ = _predict(codes, params, None)
    return {"log_prob": log_prob, "pred": pred}


def score(codes, labels, params):
    """The probe on labelled codes: a dict of `accuracy` and `nll` (the mean of -ln p[y]) over the rows whose label lies in [0, C),
    and `n`, their number -- 0-d fp64 tensors (NaN where n = 0) -- plus predict's `log_prob` and `pred`."""
    log_prob, pred, sums = _predict(codes, params, labels)
    return {"accuracy": sums[1] / sums[0], "nll": sums[2] / sums[0], "n": sums[0], "log_prob": log_prob, "pred": pred}


def model_probe(model, train_images, train_labels, test_images=None, test_labels=None, n_classes=10, labelled_per_class=0, seed=0,
                **fit_kw):
    """model.linear_probe: fit on model.transform(train_images) and score it there and, where given, on the test images.
    labelled_per_class > 0 shows the fit only the labels runners.select_labelled(train_labels, labelled_per_class, seed) picks --
    the rows a semi-supervised run with the same flag and seed trains on -- while `train_accuracy` and `train_nll` stay over ALL
    train labels.  A dict of `fit`, `train_accuracy`, `train_nll`, `n_labelled` and, with a test set, `test_accuracy`, `test_nll`."""
    codes = _codes(model.transform(train_images))
    shown = train_labels
    if int(labelled_per_class) > 0:
        from . import runners
        host = torch.as_tensor(train_labels).cpu().numpy()
        shown = torch.from_numpy(runners.select_labelled(host, int(labelled_per_class), int(seed)))
    fitted = fit(codes, shown, n_classes, **fit_kw)
    tr = score(codes, train_labels, fitted)
    n_lab = torch.as_tensor(shown)
    out = {"fit": fitted, "train_accuracy": tr["accuracy"], "train_nll": tr["nll"],
           "n_labelled": ((n_lab >= 0) & (n_lab < int(n_classes))).sum()}
    if test_images is not None:
        if test_labels is None:
            raise ValueError("test_images needs test_labels")
        te = score(_codes(model.transform(test_images)), test_labels, fitted)
        out.update(test_accuracy=te["accuracy"], test_nll=te["nll"])
    return out
