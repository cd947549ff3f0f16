"""Principal component analysis on the device (include/gmvae_hip.h gmvae_pca_*, gmvae_sym_eigh; csrc/pca.hpp): the centred
covariance in fp64 on the MFMA, a cyclic-Jacobi eigensolver in one workgroup, and for D > 128 a top-k subspace iteration around
it -- the linear baseline of the deep-clustering tables ("PCA + GMM"), the spectrum of a code, t-SNE's PCA start and the Frechet
distance.  Model independent: x is any fp32 [N, D] device tensor.  The statement is tests/pca_ref.py."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

MAX_N, MAX_D, MAX_M = 1 << 24, 4096, 128      # the library's gate (include/gmvae_hip.h)
# the defaults, pinned on the statement (tests/test_pca_cpu.py; profiles/pca_notes.md): three sweeps past the count that leaves
# offdiag <= 1e-13 at n = 128; twice the iterations that leave residual <= 1e-10 lambda_1 on every D > 128 case of the tests
N_SWEEPS, N_ITER, OVERSAMPLE = 15, 60, 8


def workspace_bytes(N, D, m):
    b = C.c_uint64()
    L.check(L.lib.gmvae_pca_workspace_bytes(int(N), int(D), int(m), C.byref(b)), "gmvae_pca_workspace_bytes")
    return b.value


def _rows(x):
    x = torch.as_tensor(x).to(L.require_gpu(), torch.float32).contiguous()
    if x.dim() != 2:
        raise ValueError("x must be [N, D]")
    return x


def start(D, m, seed=0):
    """The orthonormal start of the subspace iteration, drawn on the host: fp64 normals of torch.Generator(seed), orthonormalised
    by torch.linalg.qr on the CPU.  [D, m] fp64."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.linalg.qr(torch.randn(int(D), int(m), dtype=torch.float64, generator=g))[0].contiguous()


def fit(x, n_components=None, oversample=None, n_iter=None, n_sweeps=None, seed=0, V0=None):
    """PCA of x [N, D]: a dict of `mean` [D], `components` [k, D] (rows; each signed so that its entry of largest magnitude is
    positive), `explained_variance` [k] (eigenvalues of the covariance with divisor N - 1, descending), `explained_variance_ratio`
    (/ `total_variance` = tr C), `residual` [k], `offdiag` and `info` (0-d) -- all fp64 on the device but info (int32).
    D <= 128: every eigenpair by cyclic Jacobi (n_sweeps sweeps; `offdiag`, the largest off-diagonal entry left relative to the
    largest diagonal one, says how far it converged); residual is 0.  D > 128: the top k = n_components (default and at most 128)
    by n_iter subspace iterations on m = min(k + oversample, 128, D) vectors from the start `V0` (default: `start(D, m, seed)`),
    converged only as far as `residual` = |C v - lambda v| says.  info = j + 1 where the data's rank is below m (the iteration's
    Cholesky factorisation met pivot j that is not > 0): everything but mean and total_variance is then NaN.  Components whose
    eigenvalues (nearly) coincide are defined only up to a rotation within their eigenspace.
    Everything stays on the device; nothing synchronises with the host."""
    x = _rows(x)
    N, D = x.shape
    if not (2 <= N <= MAX_N and 1 <= D <= MAX_D):
        raise ValueError(f"x must be [N, D] with 2 <= N <= 2^24 and 1 <= D <= {MAX_D}: got [{N}, {D}]")
    k = min(D, MAX_M) if n_components is None else int(n_components)
    if not 1 <= k <= min(D, MAX_M):
        raise ValueError(f"n_components must lie in [1, min(D, {MAX_M})]: got {k} for D = {D}")
    n_iter = N_ITER if n_iter is None else int(n_iter)
    n_sweeps = N_SWEEPS if n_sweeps is None else int(n_sweeps)
    if n_iter < 0 or n_sweeps < 1:
        raise ValueError("n_iter must be >= 0 and n_sweeps >= 1")
    dev = x.device
    if D <= MAX_M:
        m, v0 = D, None
    elif V0 is not None:
        v0 = torch.as_tensor(V0).to(dev, torch.float64).contiguous()
        m = v0.shape[1] if v0.dim() == 2 else -1
        if v0.dim() != 2 or v0.shape[0] != D or not k <= m <= MAX_M:
            raise ValueError(f"V0 must be [D, m] = [{D}, m] with {k} <= m <= {MAX_M}: got {tuple(v0.shape)}")
    else:
        over = OVERSAMPLE if oversample is None else int(oversample)
        if over < 0:
            raise ValueError("oversample must be >= 0")
        m = min(k + over, MAX_M, D)
        v0 = start(D, m, seed).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    mean, comp = torch.empty(D, **f64), torch.empty(k, D, **f64)
    var, res, stats = torch.empty(k, **f64), torch.empty(k, **f64), torch.empty(4, **f64)
    info = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(workspace_bytes(N, D, m), dtype=torch.uint8, device=dev)
    L.check(L.lib.gmvae_pca_fit(L.ptr(x), N, D, k, m, n_iter, n_sweeps, L.ptr(v0), L.ptr(mean), L.ptr(comp), L.ptr(var), L.ptr(res),
                                L.ptr(stats), L.ptr(info), L.ptr(ws), L.current_stream()), "gmvae_pca_fit")
    return {"mean": mean, "components": comp, "explained_variance": var, "explained_variance_ratio": var / stats[0],
            "total_variance": stats[0], "residual": res, "offdiag": stats[1], "info": info[0]}


def _scale(fitted, whiten):
    if not whiten:
        return None
    v = fitted["explained_variance"]
    return torch.where(v > 0, v.clamp_min(torch.finfo(torch.float64).tiny).rsqrt(), torch.zeros_like(v)).contiguous()


def transform(x, fitted, whiten=False):
    """z [N, k] (fp32) = (x - mean) @ components^T, the products and sums in fp64, rounded once.  whiten: each column scaled by
    1 / sqrt(explained_variance) (0 where the variance is not > 0)."""
    x = _rows(x)
    N, D = x.shape
    comp = fitted["components"].to(x.device, torch.float64).contiguous()
    mean = fitted["mean"].to(x.device, torch.float64).contiguous()
    k = comp.shape[0]
    if comp.shape != (k, D) or mean.shape != (D,):
        raise ValueError(f"the fit is for D = {comp.shape[1]}, x has D = {D}")
    if not (1 <= N <= MAX_N and 1 <= D <= MAX_D and 1 <= k <= min(D, MAX_M)):
        raise ValueError(f"x must be [N, D] with 1 <= N <= 2^24, 1 <= D <= {MAX_D} and at most {MAX_M} components: got [{N}, {D}], k = {k}")
    scale = _scale(fitted, whiten)
    z = torch.empty(N, k, dtype=torch.float32, device=x.device)
    L.check(L.lib.gmvae_pca_transform(L.ptr(x), N, D, k, L.ptr(mean), L.ptr(comp), L.ptr(scale), L.ptr(z), L.current_stream()),
            "gmvae_pca_transform")
    return z


def inverse_transform(z, fitted, whiten=False):
    """x [N, D] (fp64) = z @ components + mean (torch; not a hot path); whiten undoes transform's scaling."""
    z = torch.as_tensor(z).to(fitted["components"].device, torch.float64)
    if whiten:
        z = z * fitted["explained_variance"].clamp_min(0).sqrt()
    return z @ fitted["components"] + fitted["mean"]


def eigh(A, n_sweeps=None):
    """The eigendecomposition of a symmetric A [n, n] (fp64; the lower triangle is read), n <= 128: a dict of `w` [n] descending,
    `V` [n, n] with the eigenvectors in its columns (signed as fit's components) and `offdiag` (0-d)."""
    A = torch.as_tensor(A).to(L.require_gpu(), torch.float64).contiguous()
    if A.dim() != 2 or A.shape[0] != A.shape[1] or not 1 <= A.shape[0] <= MAX_M:
        raise ValueError(f"A must be [n, n] with 1 <= n <= {MAX_M}: got {tuple(A.shape)}")
    n_sweeps = N_SWEEPS if n_sweeps is None else int(n_sweeps)
    if n_sweeps < 1:
        raise ValueError("n_sweeps must be >= 1")
    n = A.shape[0]
    f64 = dict(dtype=torch.float64, device=A.device)
    w, V, off, ws = torch.empty(n, **f64), torch.empty(n, n, **f64), torch.empty(1, **f64), torch.empty(n * n, **f64)
    L.check(L.lib.gmvae_sym_eigh(L.ptr(A), n, n_sweeps, L.ptr(w), L.ptr(V), L.ptr(off), L.ptr(ws), L.current_stream()), "gmvae_sym_eigh")
    return {"w": w, "V": V, "offdiag": off[0]}


def spectrum_summary(fitted):
    """The rotation-invariant counterpart of "active units": `dim90`, the smallest number of components whose cumulative
    explained_variance_ratio reaches 0.9 (k + 1 if the fitted k do not); `participation` = (sum lambda)^2 / sum lambda^2; `top_ratio`,
    the first component's share.  0-d device tensors."""
    lam, ratio = fitted["explained_variance"], fitted["explained_variance_ratio"]
    return {"dim90": (ratio.cumsum(0) < 0.9).sum() + 1, "participation": lam.sum() ** 2 / (lam * lam).sum(), "top_ratio": ratio[0]}


def frechet_distance(x, y, n_sweeps=None):
    """The Frechet (2-Wasserstein) distance between the Gaussians fitted to x [N, D] and y [M, D], D <= 128: |mu1 - mu2|^2 + tr C1 +
    tr C2 - 2 sum sqrt(max(beta, 0)), beta the eigenvalues of S^1/2 U^T C2 U S^1/2 with C1 = U S U^T (two fits and one eigh on the
    device; the [D, D] products in torch fp64).  A dict of `distance`, `mean_part`, `cov_part`, `offdiag` [2] (of x's fit and of
    the eigh).  In the units of x squared; it has a finite-sample bias and no zero point at finite N."""
    x, y = _rows(x), _rows(y)
    if x.shape[1] != y.shape[1] or x.shape[1] > MAX_M:
        raise ValueError(f"x and y must share D <= {MAX_M}: got {tuple(x.shape)} and {tuple(y.shape)}")
    fx, fy = fit(x, n_sweeps=n_sweeps), fit(y, n_sweeps=n_sweeps)
    U, S = fx["components"].T, fx["explained_variance"].clamp_min(0)
    C2 = (fy["components"].T * fy["explained_variance"]) @ fy["components"]
    Uh = U * S.sqrt()
    e = eigh(Uh.T @ C2 @ Uh, n_sweeps=n_sweeps)
    mean_part = ((fx["mean"] - fy["mean"]) ** 2).sum()
    cov_part = fx["total_variance"] + fy["total_variance"] - 2.0 * e["w"].clamp_min(0).sqrt().sum()
    return {"distance": mean_part + cov_part, "mean_part": mean_part, "cov_part": cov_part,
            "offdiag": torch.stack([fx["offdiag"], e["offdiag"]])}


def tsne_init(codes, **fit_kw):
    """scikit-learn's init="pca" for t-SNE: the first two principal components of the codes [N, 2] (fp32), scaled so that the first
    has standard deviation 1e-4.  A code of one dimension gets a zero second column."""
    codes = _rows(codes)
    f = fit(codes, n_components=min(2, codes.shape[1]), **fit_kw)
    z = transform(codes, f).double()
    N = codes.shape[0]      # (np.std's divisor is N, the eigenvalue's N - 1)
    sd = (f["explained_variance"][0] * ((N - 1) / N)).clamp_min(torch.finfo(torch.float64).tiny).sqrt()
    z = (z / sd * 1e-4).float()
    if z.shape[1] < 2:
        z = torch.cat([z, torch.zeros_like(z)], dim=1)
    return z.contiguous()


def model_latent_pca(model, images, **fit_kw):
    """model.latent_pca: fit(model.transform(images)) plus spectrum_summary's three readouts in the same dict."""
    f = fit(_rows(model.transform(images)), **fit_kw)
    f.update(spectrum_summary(f))
    return f
