"""gmvae_tsne_* (include/gmvae_hip.h; csrc/tsne.hpp) and gmvae_amd.tsne on the device against the fp64 statement
(tests/tsne_ref.py): the affinities on the issue's six shapes and at T - 1, T, T + 1 for every tile or slice constant T of tsne.hpp
(N around kTsTile = 32, kTsWave = 64, kTsBlock = 256 and around 2048 = kTsMaxSlices tiles, where a slice starts to hold several
tiles, and 4100; L around kTsDims = 64) in six regimes, whole and in row chunks; one gradient pass at two exaggerations and
two embedding scales; bit-equality of two calls; the memory contract on guarded buffers; ten iterations and a whole run against
the statement; the model and runner surface.

Gates (the project's own): every output element within 1e-4 max(1, |ref|); the gradient within 1e-4 of max |ref|; the search is
held to its root -- H_i recomputed here in fp64 from the returned beta within 1e-4 max(1, ln perp) of ln perp, and p_{j|i} from
the returned (beta, logz) within 1e-4 of the row's maximum.  Every test prints its worst figure before it asserts."""
import math

import numpy as np
import pytest
import torch

import tsne_ref as R
from arena import Arena

pytestmark = pytest.mark.gpu

SHAPES = [(5, 1, 2), (33, 3, 5), (67, 5, 10), (257, 64, 40), (300, 128, 30), (513, 8, 40)]      # (N, L, perplexity)
TILE_SHAPES = [(T + d, 4, 8) for T in (32, 64, 256) for d in (-1, 0, 1)]
# kTsDims = 64 acts on L: a partial and a whole staging round, a second round of one dimension, a third round
DIM_SHAPES = [(67, 63, 10), (67, 64, 10), (67, 65, 10), (40, 130, 8)]
# The slice constants (kTsMaxSlices = 64, kTsTargetBlocks = 1024) act through ts_slices / ts_split.  Up to N = 64 * 32 = 2048 a
# slice is one tile and a block's tile loop runs once; above it a slice holds several tiles: the loop restages the tile, resets
# its sums and folds across tiles.  2047, 2048: one tile; 2049: two; 4100: three, and more than 16 blocks of lanes, so fewer than
# kTsMaxSlices slices (61).  The last case walks two staging rounds of L as well.
BIG_SHAPES = [(2047, 4, 8), (2048, 4, 8), (2049, 4, 8), (4100, 4, 8), (2049, 65, 30)]
ALL_SHAPES = SHAPES + TILE_SHAPES + DIM_SHAPES + BIG_SHAPES
REGIMES = ["blob", "clusters", "duplicates", "scaled_up", "scaled_down", "outlier"]
sid = lambda s: "x".join(map(str, s))


def _L():
    from gmvae_amd import _lib
    return _lib


def make_codes(shape, regime):
    """fp32 codes [N, L] of a shape in a regime, and the cluster label of every row (zeros outside `clusters`)."""
    N, Lz, perp = shape
    rng = np.random.default_rng(100 * ALL_SHAPES.index(shape) + REGIMES.index(regime))
    c = rng.normal(0, 1, (N, Lz))
    lab = np.zeros(N, np.int64)
    if regime == "clusters":                        # four clusters 50 sigma apart: the cross-cluster p underflows to exactly 0
        lab = np.arange(N) % 4
        c[:, 0] += 50.0 * lab
    elif regime == "duplicates":                    # k identical rows, k fewer than the perplexity: every row keeps a root (a row
        k = min(3, math.ceil(perp) - 1)             # whose k nearest neighbours tie has H >= ln k at every beta); at perplexity 2
        c[N - k:] = c[0]                            # that allows k = 1 only: no duplicate
    elif regime == "scaled_up":                     # beta spans twelve decades between these two
        c *= 1e3
    elif regime == "scaled_down":
        c *= 1e-3
    elif regime == "outlier":                       # one point 1e3 away
        c[N // 2, 0] += 1e3
    return np.ascontiguousarray(c, np.float32), lab


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_REF = {}


def reference(shape, regime):
    """The statement's affinities of a case, computed once and left unchanged."""
    if (shape, regime) not in _REF:
        _REF[(shape, regime)] = R.affinities(make_codes(shape, regime)[0], shape[2])
    return _REF[(shape, regime)]


def gate_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.all(np.isfinite(got)):
        return math.inf
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def affinity_errs(shape, regime, beta, logz, entropy):
    ref = reference(shape, regime)
    perp = shape[2]
    errs = {k: gate_err(v, ref[k]) for k, v in (("beta", beta), ("logz", logz), ("entropy", entropy))}
    # the root, from the returned beta alone, in fp64
    _, H, _ = R.row_entropy(ref["d2"], beta.astype(np.float64))
    errs["root"] = float(np.abs(H - math.log(perp)).max() / max(1.0, math.log(perp)))
    # p_{j|i} from the returned (beta, logz)
    p = np.exp(-beta.astype(np.float64)[:, None] * ref["d2"] - logz.astype(np.float64)[:, None])
    np.fill_diagonal(p, 0.0)
    errs["cond"] = float((np.abs(p - ref["cond"]).max(axis=1) / ref["cond"].max(axis=1)).max())
    return errs


def run_affinities(c, perp, rows=None):
    from gmvae_amd import tsne
    b, lz, h = tsne.affinities(dev(c), perp, rows)
    torch.cuda.synchronize()
    return b.cpu().numpy(), lz.cpu().numpy(), h.cpu().numpy()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES + TILE_SHAPES + DIM_SHAPES, ids=sid)
def test_affinities_match_the_statement_whole_and_chunked(shape, regime):
    c, _ = make_codes(shape, regime)
    N, Lz, perp = shape
    ref = reference(shape, regime)
    assert np.abs(ref["entropy"] - math.log(perp)).max() < 1e-9          # every row of every case has a root
    if regime == "clusters" and shape in SHAPES[1:]:                     # below fp32's smallest number: exactly 0 on the device
        assert ref["P"][0, 1::4].max() < 1.4e-45 and ref["P"][0, 4::4].max() > 1e-4 / N
    whole = run_affinities(c, perp)
    errs = affinity_errs(shape, regime, *whole)
    print(shape, regime, {k: f"{v:.2e}" for k, v in errs.items()}, "beta", f"{ref['beta'].min():.3g}..{ref['beta'].max():.3g}")
    assert max(errs.values()) <= 1e-4, errs
    for rows in sorted({1, min(7, N), N // 2 + 1}):
        if N > 70 and rows == 1:
            continue
        parts = run_affinities(c, perp, rows)
        for a, b in zip(whole, parts):
            assert np.array_equal(a, b), rows                              # chunking changes no bit


def ref_gradient(shape, regime, beta32, logz32, y, alpha):
    """The statement's gradient at the P the fp32 (beta, logz) define: the inputs' rounding is not the kernel's."""
    d2 = reference(shape, regime)["d2"]
    p = np.exp(-beta32.astype(np.float64)[:, None] * d2 - logz32.astype(np.float64)[:, None])
    np.fill_diagonal(p, 0.0)
    return R.gradient((p + p.T) / (2 * shape[0]), y, alpha)


def gradient_errs(g, stats, ref):
    errs = {"grad": float(np.abs(g - ref["grad"]).max() / np.abs(ref["grad"]).max())}
    for k, v in zip(("Z", "spl", "kl", "plogp"), stats):
        errs[k] = gate_err(v, ref[k])
    return errs


GRAD_CASES = [(s, "blob") for s in SHAPES + TILE_SHAPES + DIM_SHAPES] + [((257, 64, 40), r) for r in REGIMES[1:]] + [((33, 3, 5), r) for r in REGIMES[1:]]


@pytest.mark.parametrize("shape,regime", GRAD_CASES, ids=lambda v: sid(v) if isinstance(v, tuple) else v)
def test_one_gradient_pass(shape, regime):
    from gmvae_amd import tsne
    c, _ = make_codes(shape, regime)
    N = shape[0]
    ref = reference(shape, regime)
    b32, lz32 = ref["beta"].astype(np.float32), ref["logz"].astype(np.float32)
    cd, bd, ld = dev(c), dev(b32), dev(lz32)
    for scale in (1e-4, 10.0):
        y = (scale * np.random.default_rng(N).normal(0, 1, (N, 2))).astype(np.float32)
        for alpha in (12.0, 1.0):
            g, st = tsne.gradient(cd, bd, ld, dev(y), alpha)
            g2, st2 = tsne.gradient(cd, bd, ld, dev(y), alpha)
            errs = gradient_errs(g.cpu().numpy(), st.cpu().numpy(), ref_gradient(shape, regime, b32, lz32, y, alpha))
            print(shape, regime, "scale", scale, "alpha", alpha, {k: f"{v:.2e}" for k, v in errs.items()})
            assert max(errs.values()) <= 1e-4, errs
            assert torch.equal(g, g2) and torch.equal(st, st2)                 # two calls, the same bits


# ------------------------------------------------------------------------------------- several tiles per slice (N > 2048)
def tiles_per_slice(N, lanes):
    """csrc/tsne.hpp ts_slices(lanes) and ts_split(N, .): (tiles of 32 points in a slice, slices in use)."""
    blocks = -(-lanes // 256)
    ns = min(64, max(1, -(-1024 // blocks)))
    per = -(-(-(-N // 32)) // ns) * 32
    return per // 32, -(-N // per)


def probe_rows(N):
    """The rows the statement is evaluated at: the first and last of tiles, slices and blocks, and 24 others."""
    edge = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 255, 256, 257, N // 2, N - 65, N - 64, N - 33, N - 32, N - 2, N - 1]
    return np.unique(np.concatenate([edge, np.random.default_rng(N).integers(0, N, 24)]))


@pytest.mark.parametrize("regime", ["blob", "clusters", "outlier"])
@pytest.mark.parametrize("shape", BIG_SHAPES, ids=sid)
def test_affinities_with_several_tiles_per_slice(shape, regime):
    """The affinities where a block walks more than one tile (tsne_dist stores at c0 > c_lo, restages s_c behind its barrier): the
    probe rows against the statement, every row bit-equal between the whole call and two chunkings."""
    c, _ = make_codes(shape, regime)
    N, Lz, perp = shape
    want = {2047: 1, 2048: 1, 2049: 2, 4100: 3}[N]
    assert tiles_per_slice(N, N)[0] == want and tiles_per_slice(N, 700)[0] == want      # whole call; a 700-row chunk
    rows = probe_rows(N)
    if regime == "outlier":
        rows = np.unique(np.append(rows, N // 2))
    ref = R.affinities(c, perp, rows=rows)
    assert np.abs(ref["entropy"] - math.log(perp)).max() < 1e-9
    whole = run_affinities(c, perp)
    b, lz, h = (a[rows] for a in whole)
    errs = {k: gate_err(v, ref[k]) for k, v in (("beta", b), ("logz", lz), ("entropy", h))}
    _, H, _ = R.row_entropy(ref["d2"], b.astype(np.float64), rows=rows)
    errs["root"] = float(np.abs(H - math.log(perp)).max() / max(1.0, math.log(perp)))
    with np.errstate(over="ignore"):
        p = np.exp(-b.astype(np.float64)[:, None] * ref["d2"] - lz.astype(np.float64)[:, None])
    p[np.arange(len(rows)), rows] = 0.0
    errs["cond"] = float((np.abs(p - ref["cond"]).max(axis=1) / ref["cond"].max(axis=1)).max())
    print(shape, regime, {k: f"{v:.2e}" for k, v in errs.items()}, "beta", f"{ref['beta'].min():.3g}..{ref['beta'].max():.3g}")
    assert max(errs.values()) <= 1e-4, errs
    for chunk in (700, N // 2 + 1):
        for a, b2 in zip(whole, run_affinities(c, perp, chunk)):
            assert np.array_equal(a, b2), chunk


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=sid)
def test_gradient_with_several_tiles_per_slice(shape):
    """One gradient pass where tsne_pairs walks more than one tile per block (s_c and s_meta restaged, the tile sums reset and
    folded in fp64 across tiles) against the row-blocked statement, at bandwidths that differ from row to row."""
    from gmvae_amd import tsne
    c, _ = make_codes(shape, "blob")
    N, Lz, perp = shape
    rng = np.random.default_rng(N + Lz)
    b32 = (rng.uniform(0.5, 2.0, N) * (2.0 / Lz)).astype(np.float32)
    lz32 = R.logz_at(c, b32).astype(np.float32)
    cd, bd, ld = dev(c), dev(b32), dev(lz32)
    for scale, alpha in ((10.0, 12.0), (1e-4, 1.0)) if shape == (2049, 4, 8) else ((10.0, 12.0),):      # (the statement costs seconds here)
        y = (scale * rng.normal(0, 1, (N, 2))).astype(np.float32)
        g, st = tsne.gradient(cd, bd, ld, dev(y), alpha)
        g2, st2 = tsne.gradient(cd, bd, ld, dev(y), alpha)
        errs = gradient_errs(g.cpu().numpy(), st.cpu().numpy(), R.gradient_from_codes(c, b32, lz32, y, alpha))
        print(shape, "scale", scale, "alpha", alpha, {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) <= 1e-4, errs
        assert torch.equal(g, g2) and torch.equal(st, st2)


def test_memory_contract_on_guarded_buffers():
    """Every call on arena buffers (N = 67, L = 5: no size is a multiple of a tile): the affinities change their row range of the
    three outputs and the workspace, the gradient its two outputs and the workspace, the run y, vel, gains, the history and the
    workspace -- nothing else."""
    from gmvae_amd import tsne
    L = _L()
    shape, regime = (67, 5, 10), "blob"
    N, Lz, perp = shape
    c, _ = make_codes(shape, regime)
    rows, n_iter = 24, 4
    ar = Arena("cuda", 16 << 20)
    f32 = torch.float32
    codes = ar.place("codes", c.nbytes, Lz * 4, False, f32)
    codes.copy_(torch.from_numpy(c.reshape(-1)))
    out = {k: ar.place(k, N * 4, 4, False, f32) for k in ("beta", "logz", "entropy")}
    ws = ar.place("workspace", tsne.workspace_bytes(N, Lz, rows), 16, True, torch.uint8)
    y0 = (1e-4 * np.random.default_rng(1).normal(0, 1, (N, 2))).astype(np.float32)
    st = {k: ar.place(k, N * 8, 8, False, f32) for k in ("y", "vel", "gains", "grad")}
    stats = ar.place("stats", 16, 4, False, f32)
    hist = ar.place("kl_history", n_iter * 4, 4, False, f32)
    st["y"].copy_(torch.from_numpy(y0.reshape(-1)))
    st["vel"].zero_()
    st["gains"].fill_(1.0)
    for r0 in range(0, N, rows):
        n = min(rows, N - r0)
        for k in out:
            ar.set_writable(k, [(r0 * 4, (r0 + n) * 4)])
        ar.snapshot()
        assert L.lib.gmvae_tsne_affinities(L.ptr(codes), N, Lz, float(perp), r0, n, L.ptr(out["beta"]), L.ptr(out["logz"]),
                                           L.ptr(out["entropy"]), L.ptr(ws), L.current_stream()) == 0
        ar.check()
    for k in out:
        ar.set_writable(k, False)
    errs = affinity_errs(shape, regime, *(out[k].cpu().numpy() for k in ("beta", "logz", "entropy")))
    print("arena affinities", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-4
    ar.set_writable("grad", True)
    ar.set_writable("stats", True)
    ar.snapshot()
    assert L.lib.gmvae_tsne_gradient(L.ptr(codes), N, Lz, L.ptr(out["beta"]), L.ptr(out["logz"]), L.ptr(st["y"]), 12.0,
                                     L.ptr(st["grad"]), L.ptr(stats), L.ptr(ws), L.current_stream()) == 0
    ar.check()
    ref = ref_gradient(shape, regime, out["beta"].cpu().numpy(), out["logz"].cpu().numpy(), y0, 12.0)
    errs = gradient_errs(st["grad"].view(N, 2).cpu().numpy(), stats.cpu().numpy(), ref)
    print("arena gradient", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-4
    # stats_out = NULL: the gradient alone
    ar.set_writable("stats", False)
    ar.snapshot()
    assert L.lib.gmvae_tsne_gradient(L.ptr(codes), N, Lz, L.ptr(out["beta"]), L.ptr(out["logz"]), L.ptr(st["y"]), 12.0,
                                     L.ptr(st["grad"]), None, L.ptr(ws), L.current_stream()) == 0
    ar.check()
    ar.set_writable("grad", False)
    for k in ("y", "vel", "gains", "kl_history"):
        ar.set_writable(k, True)
    ar.snapshot()
    assert L.lib.gmvae_tsne_run(L.ptr(codes), N, Lz, L.ptr(out["beta"]), L.ptr(out["logz"]), L.ptr(st["y"]), L.ptr(st["vel"]),
                                L.ptr(st["gains"]), n_iter, 2, 12.0, 50.0, L.ptr(hist), L.ptr(ws), L.current_stream()) == 0
    ar.check()
    assert all(torch.isfinite(t).all() for t in (st["y"], st["vel"], st["gains"], hist))
    # no history asked for, no iteration asked for: nothing but (y, vel, gains) / nothing at all
    ar.set_writable("kl_history", False)
    ar.snapshot()
    assert L.lib.gmvae_tsne_run(L.ptr(codes), N, Lz, L.ptr(out["beta"]), L.ptr(out["logz"]), L.ptr(st["y"]), L.ptr(st["vel"]),
                                L.ptr(st["gains"]), 1, 2, 12.0, 50.0, None, L.ptr(ws), L.current_stream()) == 0
    ar.check()
    for k in ("y", "vel", "gains", "workspace"):
        ar.set_writable(k, False)
    ar.snapshot()
    assert L.lib.gmvae_tsne_run(L.ptr(codes), N, Lz, L.ptr(out["beta"]), L.ptr(out["logz"]), L.ptr(st["y"]), L.ptr(st["vel"]),
                                L.ptr(st["gains"]), 0, 2, 12.0, 50.0, L.ptr(hist), L.ptr(ws), L.current_stream()) == 0
    ar.check()


# ------------------------------------------------------------------------------------------------------------ iterations
ITER_CASES = [((67, 5, 10), "blob"), ((67, 5, 10), "duplicates"), ((257, 64, 40), "blob"), ((257, 64, 40), "clusters"),
              ((257, 64, 40), "outlier"), ((33, 3, 5), "scaled_up"), ((33, 3, 5), "scaled_down")]
N_ITER, EX_ITERS = 10, 5
# The same statement (the search, P, ten iterations) evaluated in fp32 NumPy (tsne_ref with dtype=float32, its search bisected
# until fp32 cannot split the bracket, as the device's is) against the fp64 statement on ITER_CASES: the worst
# max |y - y_ref| / max |y_ref| and the worst |kl - ref| / max(1, |ref|) over the history and the final KL, measured on the CPU
# (profiles/tsne_notes.md lists every case, and the figures of an fp32 search that stops at |H - ln perp| <= 1e-5: 7.0e-5, 6.5e-6).
FP32_STATEMENT_Y, FP32_STATEMENT_KL = 4.90e-6, 7.89e-7
ITER_TOL_Y, ITER_TOL_KL = 4 * FP32_STATEMENT_Y, 4 * FP32_STATEMENT_KL      # 4 x: the fold order differs


def iter_init(N):
    return (1e-4 * np.random.default_rng(77 + N).normal(0, 1, (N, 2))).astype(np.float32)


def iter_errs(y, hist, ref):
    return (float(np.abs(y - ref["embedding"]).max() / np.abs(ref["embedding"]).max()),
            float((np.abs(hist - ref["kl_history"]) / np.maximum(1.0, np.abs(ref["kl_history"]))).max()))


@pytest.mark.parametrize("shape,regime", ITER_CASES, ids=lambda v: sid(v) if isinstance(v, tuple) else v)
def test_ten_iterations_match_the_statement(shape, regime):
    from gmvae_amd import tsne
    c, _ = make_codes(shape, regime)
    N, Lz, perp = shape
    ref = R.run(reference(shape, regime)["P"], iter_init(N), N_ITER, EX_ITERS)
    o = tsne.embed(dev(c), perplexity=perp, n_iter=N_ITER, exaggeration_iters=EX_ITERS, init=dev(iter_init(N)))
    ey, ek = iter_errs(o["embedding"].cpu().numpy(), o["kl_history"].cpu().numpy(), ref)
    kerr = abs(o["kl"].item() - ref["kl"]) / max(1.0, abs(ref["kl"]))
    print(shape, regime, f"y {ey:.2e} (tol {ITER_TOL_Y:.2e}) kl_history {ek:.2e} (tol {ITER_TOL_KL:.2e}) kl {kerr:.2e}")
    assert ey <= ITER_TOL_Y and ek <= ITER_TOL_KL and kerr <= ITER_TOL_KL
    again = tsne.embed(dev(c), perplexity=perp, n_iter=N_ITER, exaggeration_iters=EX_ITERS, init=dev(iter_init(N)))
    for k in ("embedding", "kl", "kl_history", "beta", "entropy"):
        assert torch.equal(o[k], again[k]), k                                  # two runs, the same bits


def test_whole_run_separates_the_clusters():
    """clusters at N = 400, L = 16, perplexity 30, the default 300 iterations: finite, the KL falls after the exaggeration ends,
    and the share of points whose nearest neighbour in the embedding carries their cluster label is at least that of the fp64
    statement's run from the same init, minus 0.02."""
    from gmvae_amd import tsne
    N, Lz, perp = 400, 16, 30.0
    rng = np.random.default_rng(400)
    lab = np.arange(N) % 4
    c = rng.normal(0, 1, (N, Lz))
    c[:, 0] += 50.0 * lab
    c = c.astype(np.float32)
    y0 = (1e-4 * rng.normal(0, 1, (N, 2))).astype(np.float32)
    o = tsne.embed(dev(c), perplexity=perp, init=dev(y0))
    y, hist = o["embedding"].cpu().numpy(), o["kl_history"].cpu().numpy()
    ref = R.run(R.affinities(c, perp)["P"], y0)
    share, share_ref = R.nn_label_share(y, lab), R.nn_label_share(ref["embedding"], lab)
    print(f"kl {o['kl'].item():.4f} (ref {ref['kl']:.4f}) at 250: {hist[250]:.4f} (ref {ref['kl_history'][250]:.4f}) "
          f"share {share:.3f} (ref {share_ref:.3f})")
    assert hist.shape == (300,) and np.isfinite(y).all() and np.isfinite(hist).all() and math.isfinite(o["kl"].item())
    assert o["kl"].item() < hist[250]
    assert share >= share_ref - 0.02


def test_default_init_is_the_philox_stream_and_the_surface():
    from gmvae_amd import tsne, utils
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    L = _L()
    c, _ = make_codes((67, 5, 10), "blob")
    a, b, other = (tsne.embed(dev(c), perplexity=10, n_iter=0, seed=s)["embedding"] for s in (3, 3, 4))
    eps = torch.empty(67, 2, device="cuda")
    L.check(L.lib.gmvae_noise_fill(L.ptr(eps), None, 67, 2, 1, 0, 3, 0, None, L.current_stream()), "noise")
    assert torch.equal(a, b) and not torch.equal(a, other) and torch.equal(a, eps * 1e-4)
    assert 0.5e-4 < a.std().item() < 2e-4
    with pytest.raises(ValueError, match="perplexity"):
        tsne.embed(dev(c), perplexity=66.0)
    with pytest.raises(ValueError, match="init"):
        tsne.embed(dev(c), perplexity=10, init=torch.zeros(66, 2))
    r = utils.reduce_dimensionality(dev(c), perplexity=10)
    assert r.shape == (67, 2) and r.is_cuda and torch.isfinite(r).all()
    x = torch.from_numpy((np.random.default_rng(2).random((48, 64)) < 0.5).astype(np.uint8)).cuda()
    for model in (create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1),
                  create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)):
        o = model.embed_latent(x, perplexity=10, n_iter=20)
        assert set(o) == {"embedding", "kl", "kl_history", "beta", "entropy"}
        assert o["embedding"].shape == (48, 2) and o["kl_history"].shape == (20,) and o["beta"].shape == (48,)
        assert all(torch.isfinite(o[k]).all() for k in o)


def test_run_eval_embeds_the_latent_code(tmp_path):
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=200", "--batch_size=40"]
    run_gmvae.main(["--mode=train"] + args)
    out = tmp_path / "embedding.npy"
    res = run_gmvae.main(["--mode=eval", "--embed_latent=64", "--tsne_iters=50", f"--embedding_out={out}"] + args)
    new = {"latent_embedding", "samples_embedding", "train/embedding_kl"}
    emb, smp = res["latent_embedding"], res["samples_embedding"]
    assert emb.shape == (64, 2) and torch.isfinite(emb).all() and math.isfinite(res["train/embedding_kl"])
    assert smp.shape == (res["samples"].shape[0], 2) and torch.isfinite(smp).all()        # 10 draws x 10 components: perplexity 40 fits
    assert np.array_equal(np.load(out), emb.cpu().numpy())
    few = run_gmvae.main(["--mode=eval", "--embed_latent=64", "--tsne_iters=5", "--num_samples=4"] + args)
    assert few["samples_embedding"] is None and few["latent_embedding"].shape == (64, 2)  # 40 draws: the perplexity does not fit
    plain = run_gmvae.main(["--mode=eval"] + args)
    assert set(plain) == set(res) - new and not new & set(plain)
    small = [a if not a.startswith("--synthetic_size") else "--synthetic_size=30" for a in args]
    with pytest.raises(ValueError, match="--embed_latent 64.*30 examples.*--tsne_perplexity"):      # refused before the pass
        run_gmvae.main(["--mode=eval", "--embed_latent=64"] + small)
