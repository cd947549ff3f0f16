"""tests/pca_cases.py pinned on the statement alone (tests/pca_ref.py), no GPU: the table's cases are ones on which the gates of
tests/test_pca.py can be asked of every component, and gmvae_amd.pca's defaults meet the criteria they were chosen by
(profiles/pca_notes.md)."""
import numpy as np
import pytest

import pca_cases as K
import pca_ref as R

SPECIAL = [("big_offset", K.big_offset), ("constant_column", K.constant_column)]


def _all():
    for shape in K.DENSE + K.ITERATIVE:
        yield K.sid(shape), K.data(shape), shape[2]
    for name, make in SPECIAL:
        yield name, make(), make().shape[1]


def test_the_subspace_path_agrees_with_eigh():
    for shape in K.ITERATIVE:
        ref = K.reference(shape)
        w, V = R.eigh(ref["covariance"])
        k = shape[2]
        err_w = np.abs(ref["explained_variance"] - w[:k]).max() / w[0]
        err_v = np.abs(ref["components"] - V.T[:k]).max()
        print(f"{shape}: eigenvalues {err_w:.3e} lambda_1, components {err_v:.3e}, residual {ref['residual'].max() / w[0]:.3e} lambda_1")
        assert ref["info"] == 0 and err_w <= 1e-12 and err_v <= 1e-10


def test_every_compared_component_is_well_separated_and_its_sign_is_stable():
    for name, x, k in _all():
        mu, C = R.moments(x)
        w, V = R.eigh(C)
        gap, margin = K.gaps(w, k).min(), K.sign_margin(V.T[:k]).min()
        print(f"{name}: the smallest relative gap {gap:.3e}, the smallest sign margin {margin:.3e}")
        assert gap > K.MIN_GAP and margin > 1e-6
    for n in K.EIGH_SIZES:
        w, V = R.eigh(K.sym(n, seed=400 + n))
        assert (K.gaps(w, n) * abs(w[0])).min() > 1e-8 * abs(w).max() and K.sign_margin(V.T).min() > 1e-6


def test_the_statement_is_insensitive_at_the_gates_scale():
    """C perturbed by 1e-15 relative and solved again: the components move by less than 1e-9 (the gate on them is 1e-8)."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for name, x, k in _all():
        mu, C = R.moments(x)
        E = rng.standard_normal(C.shape)
        w0, V0 = R.eigh(C)
        w1, V1 = R.eigh(C + 1e-15 * np.abs(C).max() * (E + E.T))
        moved = np.abs(V0.T[:k] - V1.T[:k]).max()
        worst = max(worst, moved)
        assert moved < 1e-9, (name, moved)
        assert np.abs(w0 - w1).max() <= 1e-13 * w0[0]
    print(f"the largest movement of a compared component: {worst:.3e}")


def test_the_default_sweeps_meet_their_criterion():
    """n_sweeps = 3 + the smallest count at which the round-robin sweep leaves offdiag <= 1e-13 on every n = 128 fixture."""
    fixtures = [K.reference(s)["covariance"] for s in K.DENSE if s[1] == 128] + [K.sym(128, seed=400 + 128)]
    need = 0
    for A in fixtures:
        count = next(s for s in range(1, K.N_SWEEPS + 1) if R.jacobi(A, s)[2] <= K.SWEEP_TARGET)
        w, V, off = R.jacobi(A, count)
        wr, _ = R.eigh(A)
        assert np.abs(np.sort(w)[::-1] - wr).max() <= 1e-12 * np.abs(wr).max()
        need = max(need, count)
    print(f"sweeps needed at n = 128: {need}")
    assert K.N_SWEEPS == need + 3


def test_the_round_robin_visits_every_pair_once_a_sweep():
    for n in (1, 2, 3, 7, 17, 128):
        ne = (n + 1) & ~1
        seen = set()
        for r in range(ne - 1):
            p, q = R.round_robin(n, r)
            assert len(set(p) | set(q)) == 2 * len(p)                 # disjoint within a round
            seen |= set(zip(p.tolist(), q.tolist()))
        assert seen == {(i, j) for i in range(n) for j in range(i + 1, n)}


def test_the_default_iterations_and_oversampling_meet_their_criterion():
    for shape in K.ITERATIVE:
        N, D, k, m = shape
        lam1 = np.linalg.eigvalsh(K.reference(shape)["covariance"])[-1]
        table = K.reference(shape)["residual"].max() / lam1
        half = R.fit(K.data(shape), k, m, K.N_ITER // 2, K.start(shape))["residual"].max() / lam1
        md = min(k + K.OVERSAMPLE, R.MAX_DENSE, D)
        own = R.fit(K.data(shape), k, md, K.N_ITER, R.start(D, md, seed=0))["residual"].max() / lam1
        print(f"{shape}: residual / lambda_1 = {table:.3e} at the table's m, {half:.3e} after half the iterations, {own:.3e} at m = {md}")
        assert max(table, half, own) <= K.RESIDUAL_TARGET


def test_the_rank_deficient_case_fails_where_the_table_says():
    x, V0 = K.rank_deficient()
    N, D, k, m = K.RANK_DEFICIENT
    assert np.linalg.matrix_rank(x.astype(np.float64) - x.astype(np.float64).mean(axis=0)) == 10
    ref = R.fit(x, k, m, K.N_ITER, V0)
    assert 11 <= ref["info"] <= 16 and np.isnan(ref["components"]).all() and np.isfinite(ref["mean"]).all()
    mu, Cm = R.moments(x)
    W = Cm @ V0
    with pytest.raises(np.linalg.LinAlgError):
        for _ in range(K.N_ITER):                                     # NumPy's own factorisation fails there too
            W = Cm @ (W @ np.linalg.inv(np.linalg.cholesky(W.T @ W)).T)


def test_the_package_defaults_are_the_tables():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import pca
    assert (pca.N_SWEEPS, pca.N_ITER, pca.OVERSAMPLE) == (K.N_SWEEPS, K.N_ITER, K.OVERSAMPLE)
    assert (pca.MAX_M, pca.MAX_D) == (R.MAX_DENSE, 4096)
    v = pca.start(200, 16, seed=3)
    assert v.shape == (200, 16) and v.dtype.is_floating_point and abs(v.T @ v - np.eye(16)).max().item() <= 1e-14
