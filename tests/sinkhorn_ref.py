"""The statement of gmvae_amd.sinkhorn (include/gmvae_hip.h gmvae_sinkhorn; csrc/sinkhorn.hpp): the debiased Sinkhorn divergence
(Genevay et al. 2018; Feydy et al. 2019) between two weighted samples, in longdouble where the platform has one (numpy only).

    C(u, v) = 1/2 sum_d (u_d - v_d)^2                      (from differences, in longdouble)
    softmin_e(pts, h, w)(u) = -e log sum_j w_j exp((h_j - C(u, pts_j)) / e)
    f = g = p = q = 0; for t < T, e = eps[t]:
      half A: f <- softmin(y, g, b) at x;  p <- (p + softmin(x, p, a) at x) / 2;  q <- (q + softmin(y, q, b) at y) / 2
      half B: g <- softmin(x, f, a) at y (the new f);  p and q averaged once more
    last pass, e = eps[T]: f' = softmin(y, g, b) at x, p' = softmin(x, p, a) at x, q' = softmin(y, q, b) at y, none averaged
    part_x = <a, f' - p'>, part_y = <b, g - q'>, S = part_x + part_y
    contrib_x = f' - p', contrib_y = g - q'
    marginal_err = max_i |expm1((f_i - f'_i) / eps[T])|
    schedule: eps[T] = blur^2, blur = blur_rel rms_distance(pooled); eps[0] = max((2 max_i |z_i - mean|)^2, eps[T]);
      eps[i] = eps[0] (eps[T] / eps[0])^(i / K) for i < K = T - n_final, eps[T] from i = K on
    cscale = rms_distance^2 / 2: the mean cost over the pairs of the pooled sample

The log-sum-exp takes its maximum and its sum in longdouble; the exponentials of the (non-positive) reduced arguments are taken in
fp64 -- a relative error of 1e-16 a term, seven orders below the device's gate -- because numpy's longdouble exp is thirty times
slower.  form="expanded" is the form the statement allows the device: everything fp64, the cost from the expanded square on the
rows centred by the pooled mean, clamped at 0, C_ii = 0 exactly on the symmetric problems."""
import numpy as np

LD = np.longdouble
GATE = 1e-9          # the device's gate, in units of cscale
TOL = 1e-8           # a split counts as >= the observed one from S - TOL cscale on
STORE = 1 << 22      # cost matrices up to this many entries are kept; larger ones are recomputed in row chunks each pass
BLUR_REL, N_ITER = 0.1, 200


def rms_distance(z):
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    N = z.shape[0]
    return float(np.sqrt(2.0 * N / (N - 1) * z.var(axis=0).sum()))


def cscale(z):
    return 0.5 * rms_distance(z) ** 2


def schedule(z, n_iter=N_ITER, blur=None, blur_rel=BLUR_REL, n_final=None):
    """eps [n_iter + 1] (fp64) of the pooled sample z."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    T = int(n_iter)
    n_final = T // 4 if n_final is None else int(n_final)
    blur = blur_rel * rms_distance(z) if blur is None else float(blur)
    eT = blur * blur
    r = np.sqrt(((z - z.mean(axis=0)) ** 2).sum(axis=1).max())
    e0 = max((2.0 * r) ** 2, eT)
    K = T - n_final
    i = np.arange(T + 1, dtype=np.float64)
    frac = np.minimum(i / K, 1.0) if K > 0 else np.ones(T + 1)
    return np.where(frac >= 1.0, eT, np.exp(np.log(e0) + frac * (np.log(eT) - np.log(e0))))


class Cost:
    """C [nu, nv] between the rows u and v, handed out in row chunks.  form "statement": differences in longdouble; "expanded":
    the device's form in fp64 (mean: the pooled mean; same: u is v, so C_ii = 0)."""

    def __init__(self, u, v, form, mean, same):
        self.form, self.same = form, same
        ft = LD if form == "statement" else np.float64
        self.u, self.v = np.asarray(u, dtype=np.float32).astype(ft), np.asarray(v, dtype=np.float32).astype(ft)
        if form == "expanded":
            self.u, self.v = self.u - mean, self.v - mean
            self.nu, self.nv = (self.u * self.u).sum(axis=1), (self.v * self.v).sum(axis=1)
        nu, nv = len(self.u), len(self.v)
        self.step = nu if nu * nv <= STORE else max(1, STORE // nv)
        self.kept = self.block(0, nu) if self.step == nu else None

    def block(self, lo, hi):
        if self.form == "expanded":
            c = np.maximum(0.5 * (self.nu[lo:hi, None] + self.nv[None, :]) - self.u[lo:hi] @ self.v.T, 0.0)
            if self.same:
                c[np.arange(hi - lo), np.arange(lo, hi)] = 0.0
            return c
        c = np.zeros((hi - lo, len(self.v)), dtype=LD)
        for d in range(self.u.shape[1]):
            e = self.u[lo:hi, d, None] - self.v[None, :, d]
            e *= e
            c += e
        c *= LD(0.5)
        return c

    def chunks(self):
        if self.kept is not None:
            yield 0, self.kept
            return
        for lo in range(0, len(self.u), self.step):
            yield lo, self.block(lo, min(lo + self.step, len(self.u)))


def softmin(cost, h, logw, eps):
    """-eps log sum_j exp(logw_j + (h_j - C_ij) / eps) per row i, in the cost's float type."""
    ft = cost.u.dtype
    out = np.empty(len(cost.u), dtype=ft)
    eps = ft.type(eps)
    for lo, c in cost.chunks():
        s = logw[None, :] + (h[None, :] - c) / eps
        mx = s.max(axis=1)
        s -= mx[:, None]
        e = np.exp(s.astype(np.float64)).astype(ft)
        out[lo:lo + len(c)] = -eps * (np.log(e.sum(axis=1)) + mx)
    return out


def divergence(x, y, eps, a=None, b=None, form="statement"):
    """The statement on x [n, D], y [m, D] (fp32), the schedule eps [T + 1] and the weights a [n], b [m] (None: uniform): a dict of
    f, g, p, q, contrib_x, contrib_y (fp64 arrays) and sinkhorn, part_x, part_y, marginal_err (floats)."""
    ft = LD if form == "statement" else np.float64
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n, m = len(x), len(y)
    a = np.full(n, 1.0 / n) if a is None else np.asarray(a, dtype=np.float64)
    b = np.full(m, 1.0 / m) if b is None else np.asarray(b, dtype=np.float64)
    la, lb = np.log(a.astype(ft)), np.log(b.astype(ft))
    la, lb = la - np.log(a.astype(ft).sum()), lb - np.log(b.astype(ft).sum())
    mean = np.concatenate([x, y]).astype(np.float64).mean(axis=0)
    cxy, cxx, cyy = Cost(x, y, form, mean, False), Cost(x, x, form, mean, True), Cost(y, y, form, mean, True)
    cyx = Cost(y, x, form, mean, False)
    if cxy.kept is not None:
        cyx.kept, cyx.step = cxy.kept.T, m
    f, g, p, q = np.zeros(n, dtype=ft), np.zeros(m, dtype=ft), np.zeros(n, dtype=ft), np.zeros(m, dtype=ft)
    half = ft(0.5)
    T = len(eps) - 1
    for t in range(T):
        e = eps[t]
        f = softmin(cxy, g, lb, e)
        p = half * (p + softmin(cxx, p, la, e))
        q = half * (q + softmin(cyy, q, lb, e))
        g = softmin(cyx, f, la, e)
        p = half * (p + softmin(cxx, p, la, e))
        q = half * (q + softmin(cyy, q, lb, e))
    e = eps[T]
    f1, p1, q1 = softmin(cxy, g, lb, e), softmin(cxx, p, la, e), softmin(cyy, q, lb, e)
    aw, bw = a.astype(ft) / a.astype(ft).sum(), b.astype(ft) / b.astype(ft).sum()
    part_x, part_y = (aw * (f1 - p1)).sum(), (bw * (g - q1)).sum()
    err = np.abs(np.expm1(((f - f1) / ft(e)).astype(np.float64))).max()
    d = lambda v: np.asarray(v, dtype=np.float64)
    return {"f": d(f1), "g": d(g), "p": d(p1), "q": d(q1), "contrib_x": d(f1 - p1), "contrib_y": d(g - q1),
            "sinkhorn": float(part_x + part_y), "part_x": float(part_x), "part_y": float(part_y), "marginal_err": float(err)}


def p_value(obs, null, scale):
    """(1 + #{null >= obs - TOL scale}) / P, P = len(null) + 1: the two-sample test's tie rule."""
    null = np.asarray(null, dtype=np.float64)
    return (1.0 + (null >= obs - TOL * scale).sum()) / (len(null) + 1)
