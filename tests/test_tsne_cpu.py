"""CPU-side checks of gmvae_tsne_* (include/gmvae_hip.h) and of the fp64 statement the GPU tests hold it to (tests/tsne_ref.py):
the four names are declared, exported and bound; every failing argument returns its documented code before any launch (fake
pointers, never dereferenced), in the documented order; utils.reduce_dimensionality's pass-through; the runner's flag checks;
the statement against scikit-learn's _joint_probabilities / _kl_divergence and against a finite difference of its own KL.
No compute calls."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import tsne_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_tsne_workspace_bytes", "gmvae_tsne_affinities", "gmvae_tsne_gradient", "gmvae_tsne_run"}
E_NULL, E_DIMS, E_ALIGN = -1, -2, -4
P = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def test_names_are_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\bint\s+(\w+)\s*\(", hdr))
    assert NAMES <= declared <= set(L.EXPORTS)
    raw = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and getattr(L.lib, name).argtypes is not None
    assert L.lib.gmvae_abi_version() == L.ABI_VERSION == 7


def size(L, N, Lz, rows):
    b = C.c_uint64()
    return L.lib.gmvae_tsne_workspace_bytes(N, Lz, rows, C.byref(b)), b.value


def test_workspace_size(L):
    for N in (4, 67, 1024, 10000):
        for Lz in (1, 64):
            rc1, b1 = size(L, N, Lz, 1)
            rcn, bn = size(L, N, Lz, N)
            assert rc1 == rcn == 0 and b1 % 16 == 0 and bn % 16 == 0
            assert b1 >= 2 * N * 7 * 8 + N * 8 + N * 4                  # a slice of partial sums, their fold, the gradient, a row
            assert bn - b1 >= (N - 1) * N * 4 - 256                     # the chunk of distance rows: rows * N floats
            assert size(L, N, 2 * Lz, 1)[1] == b1                       # nothing grows with L
    # O(rows * N), never N^2 unless the caller asks for every row at once
    assert size(L, 60000, 64, 1024)[1] < 60000 * 1024 * 4 + 64 * 60000 * 7 * 8 + (1 << 20)
    for bad in ((3, 8, 1), ((1 << 20) + 1, 8, 1), (8, 0, 1), (8, (1 << 16) + 1, 1), (8, 8, 0), (8, 8, 9), (-1, 8, 1)):
        assert size(L, *bad)[0] == E_DIMS, bad
    assert L.lib.gmvae_tsne_workspace_bytes(8, 8, 1, None) == E_NULL
    assert L.lib.gmvae_tsne_workspace_bytes(3, 8, 1, None) == E_DIMS     # the sizes come first


def _p(a):
    return None if a is None else C.c_void_p(a)


def affin(L, codes=P, N=64, Lz=4, perp=10.0, r0=0, rows=64, beta=P, logz=P, entropy=P, ws=P):
    return L.lib.gmvae_tsne_affinities(_p(codes), N, Lz, perp, r0, rows, _p(beta), _p(logz), _p(entropy), _p(ws), None)


def grad(L, codes=P, N=64, Lz=4, beta=P, logz=P, y=P, grad_out=P, stats=P, ws=P):
    return L.lib.gmvae_tsne_gradient(_p(codes), N, Lz, _p(beta), _p(logz), _p(y), 1.0, _p(grad_out), _p(stats), _p(ws), None)


def run(L, codes=P, N=64, Lz=4, beta=P, logz=P, y=P, vel=P, gains=P, n_iter=3, hist=P, ws=P):
    return L.lib.gmvae_tsne_run(_p(codes), N, Lz, _p(beta), _p(logz), _p(y), _p(vel), _p(gains), n_iter, 2, 12.0, 50.0, _p(hist),
                                _p(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for fn, ptrs, optional in ((affin, ("codes", "beta", "logz", "entropy", "ws"), ()),
                               (grad, ("codes", "beta", "logz", "y", "grad_out", "ws"), ("stats",)),
                               (run, ("codes", "beta", "logz", "y", "vel", "gains", "ws"), ("hist",))):
        f = lambda **kw: fn(L, **kw)
        for kw in (dict(N=3), dict(N=(1 << 20) + 1), dict(Lz=0), dict(Lz=(1 << 16) + 1), dict(N=-7)):
            assert f(**kw) == E_DIMS, (fn.__name__, kw)
        for name in ptrs:
            assert f(**{name: None}) == E_NULL, (fn.__name__, name)
            assert f(**{name: None}, N=3) == E_DIMS, (fn.__name__, name)                       # the sizes come first,
            other = ptrs[0] if name != ptrs[0] else ptrs[1]
            assert f(**{name: None, other: P + 2}) == E_NULL, (fn.__name__, name)              # then NULL, then the alignment
            assert f(**{name: P + (8 if name == "ws" else 2)}) == E_ALIGN, (fn.__name__, name)
        for name in optional:
            assert f(**{name: P + 2}) == E_ALIGN, (fn.__name__, name)
    a = lambda **kw: affin(L, **kw)
    for perp in (1.0, 0.5, 63.0, 64.0, float("nan"), -3.0):
        assert a(perp=perp) == E_DIMS, perp
    assert a(rows=0) == E_DIMS and a(rows=-1) == E_DIMS and a(r0=-1) == E_DIMS and a(r0=1, rows=64) == E_DIMS
    assert a(r0=60, rows=5) == E_DIMS and a(perp=1.0, codes=None) == E_DIMS
    assert run(L, n_iter=-1) == E_DIMS and run(L, n_iter=-1, codes=None) == E_DIMS


def test_reduce_dimensionality_passes_small_codes_through(L):
    import torch
    from gmvae_amd import utils
    for shape in ((7, 2), (7, 1), (0, 2)):
        t = torch.randn(*shape)
        assert utils.reduce_dimensionality(t) is t and utils.reduce_dimensionality(t, perplexity=5) is t
    a = np.zeros((5, 2), np.float32)
    assert utils.reduce_dimensionality(a) is a
    with pytest.raises(ValueError, match="dim"):
        utils.reduce_dimensionality(torch.randn(7, 5), dim=3)
    with pytest.raises(ValueError, match="dim"):
        utils.reduce_dimensionality(torch.randn(7, 2), dim=1)


def test_runner_flag_checks(L, monkeypatch):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--embed_latent=64", "--tsne_perplexity=20", "--tsne_iters=50"]))
    assert (ok.embed_latent, ok.tsne_perplexity, ok.tsne_iters, ok.embedding_out) == (64, 20.0, 50, None)
    plain = run_gmvae.check_args(p, p.parse_args(["--mode=eval"]))
    assert (plain.embed_latent, plain.tsne_perplexity, plain.tsne_iters) == (0, 40.0, 300)
    for bad in (["--mode=train", "--embed_latent=64"], ["--embed_latent=64"], ["--mode=eval", "--embed_latent=-1"],
                ["--mode=eval", "--embed_latent=40"],                       # the default perplexity 40 needs N > 41
                ["--mode=eval", "--embed_latent=64", "--tsne_perplexity=1"], ["--mode=eval", "--embed_latent=64", "--tsne_iters=-1"],
                ["--mode=eval", "--embedding_out=e.npy"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--embed_latent=64"]))
    run_gmvae.check_args(p, p.parse_args(["--mode=eval"]))                  # without the flag, several ranks are fine


def _case(seed=0, N=60, Lz=5):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (N, Lz)).astype(np.float32), rng.normal(0, 1.0, (N, 2))


def test_statement_agrees_with_scikit_learn():
    """tsne_ref against sklearn.manifold._t_sne at N = 60, L = 5, perplexity 10: P to 1e-3 of its maximum, the gradient and the
    KL at alpha = 1 to 1e-4 of their maxima (scikit-learn's search stops at 1e-5 in fp32; its P is floored at 1e-16)."""
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    c, y = _case()
    a = R.affinities(c, 10.0)
    Psk = squareform(_t_sne._joint_probabilities(a["d2"].astype(np.float32), 10.0, 0))
    perr = np.abs(Psk - a["P"]).max() / a["P"].max()
    g = R.gradient(a["P"], y, 1.0)
    # both sides at the statement's P, so the comparison is of the gradient and the KL alone
    kl_sk, grad_sk = _t_sne._kl_divergence(y.ravel().copy(), squareform(a["P"], checks=False), 1.0, 60, 2)
    gerr = np.abs(grad_sk.reshape(60, 2) - g["grad"]).max() / np.abs(g["grad"]).max()
    kerr = abs(kl_sk - g["kl"]) / abs(g["kl"])
    # ... and at scikit-learn's own P
    kl2, grad2 = _t_sne._kl_divergence(y.ravel().copy(), squareform(Psk, checks=False), 1.0, 60, 2)
    gerr2 = np.abs(grad2.reshape(60, 2) - g["grad"]).max() / np.abs(g["grad"]).max()
    kerr2 = abs(kl2 - g["kl"]) / abs(g["kl"])
    print(f"P {perr:.2e} grad {gerr:.2e} kl {kerr:.2e}; at scikit-learn's P: grad {gerr2:.2e} kl {kerr2:.2e}")
    assert abs(a["P"].sum() - 1.0) < 1e-12 and np.abs(a["entropy"] - math.log(10.0)).max() < 1e-10
    assert perr <= 1e-3 and max(gerr, gerr2) <= 1e-4 and max(kerr, kerr2) <= 1e-4


def test_gradient_is_the_derivative_of_the_kl():
    c, y = _case(1, 24, 3)
    P = R.affinities(c, 5.0)["P"]
    g = R.gradient(P, y, 1.0)["grad"]
    h, fd = 1e-6, np.zeros_like(y)
    for i in range(y.shape[0]):
        for d in range(2):
            yp, ym = y.copy(), y.copy()
            yp[i, d] += h
            ym[i, d] -= h
            fd[i, d] = (R.gradient(P, yp)["kl"] - R.gradient(P, ym)["kl"]) / (2 * h)
    err = np.abs(fd - g).max() / np.abs(g).max()
    print(f"finite difference {err:.2e}")
    assert err <= 1e-6
    # the row-blocked form is the same statement
    aff = R.affinities(c, 5.0)
    assert np.allclose(R.logz_at(c, aff["beta"], block=7), aff["logz"], rtol=1e-12, atol=1e-12)
    for alpha in (1.0, 12.0):
        full, blocked = R.gradient(P, y, alpha), R.gradient_from_codes(c, aff["beta"], aff["logz"], y, alpha, block=7)
        assert np.allclose(blocked["grad"], full["grad"], rtol=1e-10, atol=1e-14)
        assert all(abs(blocked[k] - full[k]) <= 1e-10 * max(1.0, abs(full[k])) for k in ("Z", "spl", "plogp", "kl"))
    sub = R.affinities(c, 5.0, rows=[3, 0, 23])
    assert sub["P"] is None and all(np.array_equal(sub[k], aff[k][[3, 0, 23]]) for k in ("beta", "logz", "entropy", "cond", "d2"))
    # exaggeration scales the attractive part alone: grad(alpha) - grad(1) = 4 (alpha - 1) sum_j p w (y_i - y_j)
    dy = y[:, None] - y[None]
    w = 1 / (1 + (dy ** 2).sum(-1))
    attr = 4 * np.einsum("ij,ijd->id", P * w, dy)
    assert np.allclose(R.gradient(P, y, 12.0)["grad"] - g, 11 * attr, rtol=1e-10, atol=1e-14)


def test_statement_handles_zeros_and_the_update():
    # two far clusters: the cross-cluster p underflows to exactly 0 and contributes 0 to the KL
    rng = np.random.default_rng(3)
    c = np.concatenate([rng.normal(0, 1, (12, 4)), rng.normal(0, 1, (12, 4)) + 200.0]).astype(np.float32)
    a = R.affinities(c, 4.0)
    assert (a["P"][:12, 12:] == 0).all() and np.isfinite(R.gradient(a["P"], rng.normal(0, 1, (24, 2)))["kl"])
    y, vel, gains = np.zeros((2, 2)), np.array([[1.0, -1.0], [0.0, 2.0]]), np.array([[1.0, 1.0], [1.0, 0.0125]])
    g = np.array([[-1.0, -1.0], [3.0, 1.0]])
    y2, v2, g2 = R.update(y, vel, gains, g, 0.5, 10.0)
    assert np.allclose(g2, [[1.2, 0.8], [0.8, 0.01]]) and np.allclose(v2, 0.5 * vel - 10.0 * g2 * g) and np.allclose(y2, v2)
