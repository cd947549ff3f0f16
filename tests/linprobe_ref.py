"""The fp64 statement of gmvae_amd.linprobe (include/gmvae_hip.h gmvae_linprobe_*; csrc/linprobe.hpp): multinomial logistic
regression on frozen codes, fitted by FISTA in the fixed metric of Boehning's bound.  numpy only.

Inputs: codes x [N, L] (fp32), labels y [N] (a label outside [0, C) marks the row unlabelled: weight 0), l2 = lambda > 0, n_iter.
  p_n = softmax((x_n - xbar) W + b),  f(W, b) = -(1/n) sum_labelled ln p_n[y_n] + (lambda / 2) |W|_F^2,  xbar = the labelled mean
  A = 1/2 (1/n) sum_labelled (x_n - xbar)(x_n - xbar)^T + lambda I      (the Hessian of f in W is <= I_C (x) A, in b <= 1/2 I; the
                                                                        centring decouples the two blocks)
  Theta_0 = V_0 = 0, t_0 = 1; per iteration, at the extrapolated point V:
    G_W = (1/n) sum (x_n - xbar)^T (p_n(V) - e_{y_n}) + lambda V_W,  G_b = (1/n) sum (p_n(V) - e_{y_n})
    Theta' = (V_W - A^-1 G_W, V_b - 2 G_b);  t' = (1 + sqrt(1 + 4 t^2)) / 2, beta = (t - 1) / t';  V' = Theta' + beta (Theta' - Theta)
Outputs: W [L, C], the un-centred bias b - xbar W [C], loss_history[it] = f(V_it), grad_max = max |G| at the last evaluated point
(NaN where nothing was evaluated: n_iter = 0).  A pivot of A's Cholesky factorisation that is not > 0 gives info = j + 1, W = b = 0
and a NaN history; no labelled row gives info = -1 and the same."""
import math

import numpy as np


def betas(n_iter):
    """The extrapolation weights beta_0 .. beta_{n_iter - 1}, in fp64 (beta_0 = 0)."""
    out, t = [], 1.0
    for _ in range(int(n_iter)):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / t1)
        t = t1
    return out


def labelled(y, C):
    y = np.asarray(y).astype(np.int64)
    return (y >= 0) & (y < int(C))


def log_softmax(logits, exp_dtype=np.float64):
    """Row-wise, the maximum subtracted; exp_dtype = float32 rounds the exponentials (and their arguments) as the device does."""
    m = logits.max(axis=1, keepdims=True)
    e = np.exp((logits - m).astype(exp_dtype)).astype(np.float64)
    s = e.sum(axis=1, keepdims=True)
    return (logits - m) - np.log(s), e / s


def cholesky_info(A):
    """(the lower factor, 0) or (None, j + 1) for the first pivot j that is not > 0."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    for j in range(n):
        p = A[j, j]
        if not p > 0.0:
            return None, j + 1
        c = math.sqrt(p)
        A[j + 1:, j] /= c
        A[j, j] = c
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A), 0


def metric(x, y, C, l2):
    """(n, xbar [L], A [L, L]) of the labelled rows."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    lab = labelled(y, C)
    n = int(lab.sum())
    xl = x[lab]
    xbar = xl.sum(axis=0) / max(n, 1)
    xc = xl - xbar
    A = 0.5 * (xc.T @ xc) / max(n, 1) + float(l2) * np.eye(x.shape[1])
    return n, xbar, A


def objective(x, y, C, l2, W, b, xbar=None):
    """f at (W, b) of the centred model (xbar None: of the un-centred one)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    lab = labelled(y, C)
    yl = np.asarray(y).astype(np.int64)[lab]
    xl = x[lab] - (0.0 if xbar is None else xbar)
    lp, _ = log_softmax(xl @ W + b)
    return -lp[np.arange(len(yl)), yl].mean() + 0.5 * float(l2) * (W * W).sum()


def fit(x, y, C, l2=1e-3, n_iter=300, exp_dtype=np.float64, theta_history=False):
    """A dict of W [L, C], b [C] (un-centred), loss_history [n_iter], grad_max, info, and the centred pieces xbar, b_centred;
    theta_history: also `thetas`, the list of (Theta_W, Theta_b centred) after every iteration."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    N, L = x.shape
    C, n_iter, l2 = int(C), int(n_iter), float(l2)
    lab = labelled(y, C)
    yl = np.asarray(y).astype(np.int64)[lab]
    n, xbar, A = metric(x, y, C, l2)
    out = {"W": np.zeros((L, C)), "b": np.zeros(C), "loss_history": np.full(n_iter, np.nan), "grad_max": float("nan"), "info": 0,
           "xbar": xbar, "b_centred": np.zeros(C), "n": n}
    if n == 0:
        out["info"] = -1
        return out
    chol, info = cholesky_info(A)
    if info:
        out["info"] = info
        return out
    Winv = np.linalg.solve(chol, np.eye(L))      # C^-1
    Ainv = Winv.T @ Winv
    xc = x[lab] - xbar
    E = np.zeros((n, C))
    E[np.arange(n), yl] = 1.0
    ThW, Thb = np.zeros((L, C)), np.zeros(C)
    VW, Vb = ThW.copy(), Thb.copy()
    thetas = []
    for it, beta in enumerate(betas(n_iter)):
        lp, p = log_softmax(xc @ VW + Vb, exp_dtype)
        out["loss_history"][it] = -lp[np.arange(n), yl].mean() + 0.5 * l2 * (VW * VW).sum()
        R = p - E
        GW = xc.T @ R / n + l2 * VW
        Gb = R.sum(axis=0) / n
        out["grad_max"] = float(max(np.abs(GW).max(), np.abs(Gb).max()))
        nW, nb = VW - Ainv @ GW, Vb - 2.0 * Gb
        VW, Vb = nW + beta * (nW - ThW), nb + beta * (nb - Thb)
        ThW, Thb = nW, nb
        if theta_history:
            thetas.append((ThW.copy(), Thb.copy()))
    out.update(W=ThW, b=Thb - xbar @ ThW, b_centred=Thb)
    if theta_history:
        out["thetas"] = thetas
    return out


def predict(x, W, b, y=None, C=None):
    """log_prob [N, C], pred [N] (the first maximal index) and the three sums over the labelled rows -- count, correct,
    sum -ln p[y] -- (zeros where y is None)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    lp, _ = log_softmax(x @ np.asarray(W, dtype=np.float64) + np.asarray(b, dtype=np.float64))
    pred = lp.argmax(axis=1)
    sums = np.zeros(3)
    if y is not None:
        lab = labelled(y, lp.shape[1] if C is None else C)
        yl = np.asarray(y).astype(np.int64)[lab]
        sums = np.array([lab.sum(), (pred[lab] == yl).sum(), -lp[lab][np.arange(len(yl)), yl].sum()], dtype=np.float64)
    return {"log_prob": lp, "pred": pred, "sums": sums}


def clusters(N, L, C, seed=0, sep=4.0, unlabelled=0.3, scale=1.0):
    """The tests' data: C Gaussian clusters with centres of scale `sep`, a share of the rows unlabelled (-1).  x fp32 [N, L], y int32 [N]
    (the labels as fit sees them), y_true int32 [N]."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, L)) * sep
    y_true = (np.arange(N) % C).astype(np.int32)
    rng.shuffle(y_true)
    x = ((centres[y_true] + rng.standard_normal((N, L))) * scale).astype(np.float32)
    y = y_true.copy()
    y[rng.random(N) < unlabelled] = -1
    if not labelled(y, C).any():
        y[0] = y_true[0]
    return x, y, y_true
