"""The fp64 statement of gmvae_tsne_* (include/gmvae_hip.h) in NumPy -- a plain module shared by tests/test_tsne_cpu.py and
tests/test_tsne.py.  Dense [N, N] arrays (row blocks of them in logz_at and gradient_from_codes): it is the statement, not an
implementation.  Every function takes `dtype`
so that the same statement can be evaluated in fp32 (the yardstick for the iteration test's tolerance).

    d2_ij = sum_d (c_id - c_jd)^2                                        (difference form)
    p_{j|i} = exp(-beta_i d2_ij - lz_i), lz_i = logsumexp_{j != i}(-beta_i d2_ij), H_i = lz_i + beta_i sum_j p_{j|i} d2_ij = ln perp
    p_ij = (p_{j|i} + p_{i|j}) / 2N, p_ii = 0
    w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij
    grad_i = 4 sum_j (alpha p_ij - w_ij / Z) w_ij (y_i - y_j);  KL = sum p ln p - sum p ln w + ln Z  (p = 0 contributes 0)
    update: scikit-learn's _gradient_descent step, no recentring."""
import numpy as np


def sqdist(c, dtype=np.float64, rows=None):
    """d2 [N, N], or its rows `rows` [len(rows), N]."""
    c = np.asarray(c, dtype)
    d = (c if rows is None else c[np.asarray(rows)])[:, None, :] - c[None, :, :]
    return np.einsum("ijd,ijd->ij", d, d)


def row_entropy(d2, beta, dtype=np.float64, rows=None):
    """(logz, H, p_{j|i} with p_{i|i} = 0) at the given beta: of every point, d2 being [N, N], or of the points `rows`, d2 being
    their rows [len(rows), N]."""
    d2, beta = np.asarray(d2, dtype), np.asarray(beta, dtype)
    own = np.arange(d2.shape[0]) if rows is None else np.asarray(rows)
    off = np.arange(d2.shape[1])[None, :] != own[:, None]
    x = np.where(off, -beta[:, None] * d2, -np.inf)
    m = x.max(axis=1)
    e = np.exp(x - m[:, None])
    s = e.sum(axis=1)
    lz = m + np.log(s)
    p = e / s[:, None]
    # H = ln S - sum x' e^x' / S with x' = x - m: the entropy of softmax(x), free of the cancellation in lz + beta sum p d2
    xs = np.where(off, x - m[:, None], 0.0)
    H = np.log(s) - (xs * e).sum(axis=1) / s
    return lz, H, p


def affinities(c, perplexity, tol=1e-12, max_halvings=200, dtype=np.float64, rows=None):
    """dict(beta, logz, entropy [N], cond = p_{j|i} [N, N], P = p_ij [N, N], d2); with `rows`, the same for those points alone
    ([len(rows)] and [len(rows), N]; P, which needs every row, is None).  The root of H_i(beta) = ln perplexity, by
    bracketing from beta = 1 and bisection, to `tol` or until the dtype cannot split the bracket (the statement is the root, not
    the path to it)."""
    d2 = sqdist(c, dtype, rows)
    R, N = d2.shape
    target = np.log(dtype(perplexity))
    beta = np.ones(R, dtype)
    lo, hi = np.zeros(R, dtype), np.full(R, np.inf, dtype)
    for _ in range(400 + max_halvings):
        lz, H, p = row_entropy(d2, beta, dtype, rows)
        diff = H - target
        done = np.abs(diff) <= tol
        if done.all():
            break
        up = (diff > 0) & ~done
        dn = (diff <= 0) & ~done
        lo = np.where(up, beta, lo)
        hi = np.where(dn, beta, hi)
        nb = np.where(up, np.where(np.isinf(hi), beta * 2, (beta + hi) / 2), np.where(lo == 0, beta / 2, (lo + beta) / 2))
        nb = np.where(done, beta, nb)
        if np.array_equal(nb, beta):
            break
        beta = nb
    lz, H, p = row_entropy(d2, beta, dtype, rows)
    P = (p + p.T) / dtype(2 * N) if rows is None else None
    return dict(beta=beta, logz=lz, entropy=H, cond=p, P=P, d2=d2)


def plogp(P):
    nz = P > 0
    return (P[nz] * np.log(P[nz])).sum()


def gradient(P, y, alpha=1.0, dtype=np.float64):
    """dict(grad [N, 2], Z, spl = sum p ln w, kl, plogp) at the embedding y."""
    P, y = np.asarray(P, dtype), np.asarray(y, dtype)
    N = y.shape[0]
    dy = y[:, None, :] - y[None, :, :]
    w = 1 / (1 + np.einsum("ijd,ijd->ij", dy, dy))
    np.fill_diagonal(w, 0)
    Z = w.sum()
    coef = (dtype(alpha) * P - w / Z) * w
    grad = 4 * np.einsum("ij,ijd->id", coef, dy)
    off = ~np.eye(N, dtype=bool)
    spl = (P[off] * np.log(w[off])).sum()
    pl = plogp(P)
    return dict(grad=grad, Z=Z, spl=spl, plogp=pl, kl=pl - spl + np.log(Z))


def logz_at(c, beta, block=128):
    """lz_i = logsumexp_{j != i}(-beta_i d2_ij) [N] at a given beta, a block of rows at a time."""
    c, beta = np.asarray(c, np.float64), np.asarray(beta, np.float64)
    lz = np.empty(c.shape[0])
    for r0 in range(0, c.shape[0], block):
        rows = np.arange(r0, min(r0 + block, c.shape[0]))
        lz[rows] = row_entropy(sqdist(c, rows=rows), beta[rows], rows=rows)[0]
    return lz


def gradient_from_codes(c, beta, logz, y, alpha=1.0, block=128):
    """gradient()'s dict at the P the given (beta, logz) define, p_{j|i} = exp(-beta_i d2_ij - logz_i), a block of rows at a time:
    the same statement without an [N, N] array, for the sizes at which the kernels walk several tiles per slice."""
    c, beta, logz, y = (np.asarray(a, np.float64) for a in (c, beta, logz, y))
    N = c.shape[0]
    grad, Z, spl, pl = np.zeros((N, 2)), 0.0, 0.0, 0.0
    attr, rep = np.zeros((N, 2)), np.zeros((N, 2))
    for r0 in range(0, N, block):
        rows = np.arange(r0, min(r0 + block, N))
        d2 = sqdist(c, rows=rows)
        off = np.arange(N)[None, :] != rows[:, None]
        with np.errstate(over="ignore"):
            P = np.where(off, (np.exp(-beta[rows, None] * d2 - logz[rows, None]) + np.exp(-beta[None, :] * d2 - logz[None, :])) / (2 * N), 0.0)
        dy = y[rows, None, :] - y[None, :, :]
        w = np.where(off, 1 / (1 + np.einsum("ijd,ijd->ij", dy, dy)), 0.0)
        attr[rows] = np.einsum("ij,ijd->id", P * w, dy)
        rep[rows] = np.einsum("ij,ijd->id", w * w, dy)
        Z += w.sum()
        spl += (P[off] * np.log(w[off])).sum()
        pl += plogp(P)
    grad = 4 * (alpha * attr - rep / Z)
    return dict(grad=grad, Z=Z, spl=spl, plogp=pl, kl=pl - spl + np.log(Z))


def update(y, vel, gains, grad, momentum, lr, dtype=np.float64):
    inc = vel * grad < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    vel = dtype(momentum) * vel - dtype(lr) * gains * grad
    return y + vel, vel, gains


def default_lr(N):
    return max(N / 48.0, 50.0)


def run(P, y0, n_iter=300, exaggeration_iters=250, exaggeration=12.0, lr=None, dtype=np.float64):
    """dict(embedding, kl (at the embedding), kl_history [n_iter]: the KL each iteration started from)."""
    P = np.asarray(P, dtype)
    y = np.array(y0, dtype)
    lr = default_lr(y.shape[0]) if lr is None else lr
    vel, gains = np.zeros_like(y), np.ones_like(y)
    hist = np.zeros(n_iter, dtype)
    for it in range(n_iter):
        early = it < exaggeration_iters
        g = gradient(P, y, exaggeration if early else 1.0, dtype)
        hist[it] = g["kl"]
        y, vel, gains = update(y, vel, gains, g["grad"], 0.5 if early else 0.8, lr, dtype)
    return dict(embedding=y, kl=gradient(P, y, 1.0, dtype)["kl"], kl_history=hist)


def nn_label_share(y, labels):
    """The share of points whose nearest neighbour in y carries their label."""
    d = sqdist(y)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(axis=1)] == labels).mean())
