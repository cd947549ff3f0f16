"""gmvae_pca_*, gmvae_sym_eigh (include/gmvae_hip.h; csrc/pca.hpp) and gmvae_amd.pca on the device against the fp64 statement
(tests/pca_ref.py) on every row of tests/pca_cases.py: the dense path, the subspace iteration, the special data, the solver on its
own, transform and whitening, the Frechet distance, bit-equality and stream order, the gates' refusals, and the t-SNE, model and
runner surface.

Gates (tests/pca_cases.py): mean, explained_variance, total_variance within 1e-9 of the tensor's own maximum magnitude in the
statement (the project's fp64 gate); every entry of every component within 1e-8 (tests/test_pca_cpu.py: every compared eigenvalue
is more than 1e-6 lambda_1 from its neighbours, so none is left out); offdiag <= 1e-12 at the defaults; residual within 1e-9
lambda_1 of the statement's; transform within 1e-6 max |ref|; the Frechet distance within 1e-9 (tr C1 + tr C2).  Every test prints
its worst figure before it asserts; the worst measured multiples are in profiles/pca_notes.md."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pca_cases as K
import pca_ref as R

pytestmark = pytest.mark.gpu


def gate(name, got, ref, tol=K.GATE, top=None):
    """The worst |got - ref| in units of the gate, tol max |ref| (or tol `top`); printed, then asserted <= 1."""
    got = np.asarray(got.cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref).max()
    top = np.abs(ref).max() if top is None else top
    print(f"  {name}: max |got - ref| = {err:.3e}, scale {top:.3e}, {err / (tol * top) if top > 0 else 0.0:.3e} of the gate")
    assert err <= tol * top, (name, err, top)


def check_fit(got, ref, offdiag=True):
    assert int(got["info"].item()) == ref["info"] == 0
    lam1 = ref["explained_variance"][0]
    gate("mean", got["mean"], ref["mean"])
    gate("total_variance", got["total_variance"], ref["total_variance"])
    gate("explained_variance", got["explained_variance"], ref["explained_variance"])
    gate("explained_variance_ratio", got["explained_variance_ratio"], ref["explained_variance_ratio"])
    gate("residual", got["residual"], ref["residual"], top=lam1)
    gate("components", got["components"], ref["components"], tol=K.GATE_COMPONENTS, top=1.0)
    if offdiag:
        print(f"  offdiag: {got['offdiag'].item():.3e}")
        assert 0.0 <= got["offdiag"].item() <= K.GATE_OFFDIAG


@pytest.mark.parametrize("shape", K.DENSE, ids=K.sid)
def test_the_dense_path_matches_the_statement(shape):
    from gmvae_amd import pca
    print(f"{shape}:")
    got = pca.fit(K.data(shape), n_components=shape[2])
    check_fit(got, K.reference(shape))
    assert not got["residual"].any().item()


@pytest.mark.parametrize("shape", K.ITERATIVE, ids=K.sid)
def test_the_subspace_iteration_matches_the_statement(shape):
    from gmvae_amd import pca
    print(f"{shape}:")
    got = pca.fit(K.data(shape), n_components=shape[2], V0=torch.from_numpy(K.start(shape)))
    check_fit(got, K.reference(shape))
    # the defaults' own start (torch's generator): the same eigenpairs, by the statement's eigh of the full covariance
    ref = K.reference(shape)
    w, V = R.eigh(ref["covariance"])
    own = pca.fit(K.data(shape), n_components=shape[2])
    gate("explained_variance, default start", own["explained_variance"], w[:shape[2]])
    gate("components, default start", own["components"], V.T[:shape[2]], tol=K.GATE_COMPONENTS, top=1.0)
    print(f"  residual / lambda_1, default start: {own['residual'].max().item() / w[0]:.3e}")
    assert own["residual"].max().item() <= K.RESIDUAL_TARGET * w[0]


def test_an_offset_of_1e4_is_centred_before_the_product():
    from gmvae_amd import pca
    x = K.big_offset()
    assert np.abs(x).min() > 9e3
    check_fit(pca.fit(x), R.fit(x))


def test_a_constant_column_has_an_exactly_zero_row_and_column():
    from gmvae_amd import pca
    x = K.constant_column()
    got, ref = pca.fit(x), R.fit(x)
    check_fit(got, ref)
    assert got["mean"][3].item() == 2.5
    assert got["explained_variance"][5].item() == 0.0            # the sixth eigenpair: e_3 with eigenvalue exactly 0
    assert torch.equal(got["components"][5].cpu(), torch.eye(6, dtype=torch.float64)[3])
    assert not got["components"][:5, 3].any().item()


def test_equal_rows_give_a_zero_spectrum_and_identity_components():
    from gmvae_amd import pca
    x = K.equal_rows()
    got = pca.fit(x)
    assert got["info"].item() == 0 and got["offdiag"].item() == 0.0 and got["total_variance"].item() == 0.0
    assert not got["explained_variance"].any().item()
    assert torch.equal(got["components"].cpu(), torch.eye(5, dtype=torch.float64))
    assert torch.equal(got["mean"].cpu(), torch.from_numpy(x[0].astype(np.float64)))
    z = pca.transform(x, got, whiten=True)                       # whitening a zero variance gives 0, not inf
    assert not z.any().item()


def test_a_rank_below_m_is_reported_not_papered_over():
    from gmvae_amd import pca
    x, V0 = K.rank_deficient()
    N, D, k, m = K.RANK_DEFICIENT
    got = pca.fit(x, n_components=k, V0=torch.from_numpy(V0))
    ref = R.fit(x, k, m, K.N_ITER, V0)
    print(f"info: device {got['info'].item()}, statement {ref['info']}")
    assert 11 <= got["info"].item() <= 16 and 11 <= ref["info"] <= 16
    for key in ("components", "explained_variance", "explained_variance_ratio", "residual", "offdiag"):
        assert torch.isnan(got[key]).all().item(), key
    gate("mean", got["mean"], ref["mean"])
    gate("total_variance", got["total_variance"], ref["total_variance"])


@pytest.mark.parametrize("n", K.EIGH_SIZES)
def test_eigh(n):
    from gmvae_amd import pca
    print(f"n = {n}:")
    d = np.random.default_rng(n).permutation(n).astype(np.float64) - n // 2       # a diagonal input: no rotation, exact output
    if n > 1:
        d[0] = d[1]                                                                # (one tie: broken by the original index)
    e = pca.eigh(np.diag(d))
    order = np.argsort(-d, kind="stable")
    assert np.array_equal(e["w"].cpu().numpy(), d[order]) and e["offdiag"].item() == 0.0
    assert np.array_equal(e["V"].cpu().numpy(), np.eye(n)[:, order])
    e = pca.eigh(2.0 * np.eye(n))                                                 # repeated eigenvalues: the decomposition, not the vectors
    V, w = e["V"].cpu().numpy(), e["w"].cpu().numpy()
    print(f"  2 I: |V^T V - I| = {np.abs(V.T @ V - np.eye(n)).max():.3e}, |A V - V w| = {np.abs(2.0 * V - V * w).max():.3e}")
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-13 and np.abs(2.0 * V - V * w).max() <= 1e-13 * 2.0
    A = K.sym(n, seed=400 + n)
    wr, Vr = R.eigh(A)
    e = pca.eigh(np.tril(A) + np.triu(np.full((n, n), 7.0), 1))                   # the upper triangle is not read
    V, w = e["V"].cpu().numpy(), e["w"].cpu().numpy()
    gate("w", w, wr)
    assert (np.diff(w) <= 0).all()
    norm = np.abs(wr).max()                                                        # |A|_2
    print(f"  offdiag {e['offdiag'].item():.3e}, |V^T V - I| = {np.abs(V.T @ V - np.eye(n)).max():.3e}, "
          f"|A V - V w| = {np.abs(A @ V - V * w).max():.3e}")
    assert e["offdiag"].item() <= K.GATE_OFFDIAG
    assert np.abs(V.T @ V - np.eye(n)).max() <= 1e-13 and np.abs(A @ V - V * w).max() <= 1e-13 * norm
    gate("V", V, Vr, tol=K.GATE_COMPONENTS, top=1.0)
    assert (V[np.abs(V).argmax(axis=0), np.arange(n)] > 0).all()                  # the sign rule


@pytest.mark.parametrize("shape", [(37, 3, 3), (403, 64, 10), (1031, 128, 128), (300, 784, 16, 32), (150, 1040, 4, 12)], ids=K.sid)
def test_transform_and_whitening(shape):
    from gmvae_amd import pca
    x, ref = K.data(shape), K.reference(shape)
    got = pca.fit(x, n_components=shape[2], V0=torch.from_numpy(K.start(shape)) if len(shape) == 4 else None)
    held = {k: got[k].cpu().numpy() for k in ("mean", "components", "explained_variance")}
    print(f"{shape}:")
    gate("transform", pca.transform(x, got), R.transform(x, held), tol=K.GATE_TRANSFORM)
    gate("whitened", pca.transform(x, got, whiten=True), R.transform(x, held, whiten=True), tol=K.GATE_TRANSFORM)
    gate("transform of the statement's fit", pca.transform(x, {k: torch.from_numpy(v) for k, v in ref.items() if k in held}),
         R.transform(x, ref), tol=K.GATE_TRANSFORM)
    one = pca.transform(x[:1], got)                              # a single row
    gate("one row", one, R.transform(x[:1], held), tol=K.GATE_TRANSFORM, top=np.abs(R.transform(x, held)).max())
    if shape[2] == shape[1]:                                     # k = D: the inverse gives x back
        back = pca.inverse_transform(pca.transform(x, got), got)
        gate("inverse_transform(transform(x))", back, x.astype(np.float64), tol=K.GATE_TRANSFORM)
        back = pca.inverse_transform(pca.transform(x, got, whiten=True), got, whiten=True)
        gate("... whitened", back, x.astype(np.float64), tol=K.GATE_TRANSFORM)


def test_frechet_distance():
    from gmvae_amd import pca
    for D, seed in ((5, 1), (64, 2), (128, 3)):
        x = R.fixture(400 + D, D, decay=0.95, seed=500 + seed)
        y = (1.3 * R.fixture(300 + D, D, decay=0.9, seed=600 + seed) + 0.2).astype(np.float32)
        rd, rm, rc = R.frechet(x, y)
        top = np.trace(R.moments(x)[1]) + np.trace(R.moments(y)[1])
        got = pca.frechet_distance(x, y)
        print(f"D = {D}: distance {got['distance'].item():.12e}, statement {rd:.12e}")
        gate("distance", got["distance"], rd, top=top)
        gate("mean_part", got["mean_part"], rm, top=top)
        gate("cov_part", got["cov_part"], rc, top=top)
        assert got["offdiag"].shape == (2,) and (got["offdiag"] <= K.GATE_OFFDIAG).all().item()
        same = pca.frechet_distance(x, x)
        print(f"  frechet(x, x) = {same['distance'].item():.3e}, the bound {K.GATE * 2 * np.trace(R.moments(x)[1]):.3e}")
        assert abs(same["distance"].item()) <= K.GATE * 2 * np.trace(R.moments(x)[1])
    with pytest.raises(ValueError):
        pca.frechet_distance(np.zeros((4, 129), np.float32), np.zeros((4, 129), np.float32))


def test_two_runs_give_the_same_bits_and_fit_and_transform_follow_the_stream():
    from gmvae_amd import pca
    for shape in ((1031, 128, 128), (600, 200, 8, 16)):
        xd = torch.from_numpy(K.data(shape)).cuda()
        v0 = torch.from_numpy(K.start(shape)).cuda() if len(shape) == 4 else None
        a = pca.fit(xd, n_components=shape[2], V0=v0)
        za = pca.transform(xd, a, whiten=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                            # fit, then transform, enqueued on one stream with nothing in between
            b = pca.fit(xd, n_components=shape[2], V0=v0)
            zb = pca.transform(xd, b, whiten=True)
        side.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (shape, k)
        assert torch.equal(za, zb)
        check_fit(b, K.reference(shape))
    A = torch.from_numpy(K.sym(128, 7)).cuda()
    e1, e2 = pca.eigh(A), pca.eigh(A)
    assert all(torch.equal(e1[k], e2[k]) for k in e1)


def test_the_gates_refuse():
    from gmvae_amd import _lib as L, pca
    E_DIMS = -2
    b = C.c_uint64()
    ws = L.lib.gmvae_pca_workspace_bytes
    for N, D, m in ((1, 4, 4), ((1 << 24) + 1, 4, 4), (10, 0, 1), (10, 4097, 8), (10, 64, 32), (10, 200, 129), (10, 200, 0), (10, 130, 131)):
        assert ws(N, D, m, C.byref(b)) == E_DIMS, (N, D, m)
    assert ws(1 << 24, 4096, 128, C.byref(b)) == 0 and b.value > 0 and ws(2, 1, 1, C.byref(b)) == 0
    x = torch.zeros(10, 200, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    out = [torch.empty(200, **f64), torch.empty(8 * 200, **f64), torch.empty(8, **f64), torch.empty(8, **f64), torch.empty(4, **f64)]
    v0, wsb = torch.zeros(200, 16, **f64), torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def call(N=10, D=200, k=8, m=16, n_iter=1, n_sweeps=1, V0=v0):
        return L.lib.gmvae_pca_fit(L.ptr(x), N, D, k, m, n_iter, n_sweeps, L.ptr(V0), *[L.ptr(o) for o in out], None, L.ptr(wsb), None)
    assert call(k=0) == E_DIMS and call(k=17) == E_DIMS and call(n_iter=-1) == E_DIMS and call(n_sweeps=0) == E_DIMS and call(N=1) == E_DIMS
    assert call(D=100, m=16) == E_DIMS and call(V0=None) == -1
    assert L.lib.gmvae_pca_transform(L.ptr(x), 10, 200, 129, L.ptr(out[0]), L.ptr(out[1]), None, L.ptr(x), None) == E_DIMS
    assert L.lib.gmvae_sym_eigh(L.ptr(v0), 129, 1, L.ptr(out[0]), L.ptr(out[1]), None, L.ptr(wsb), None) == E_DIMS
    assert L.lib.gmvae_sym_eigh(L.ptr(v0), 4, 0, L.ptr(out[0]), L.ptr(out[1]), None, L.ptr(wsb), None) == E_DIMS
    for bad in (dict(x=np.zeros((1, 4), np.float32)), dict(x=np.zeros((5, 4097), np.float32)), dict(x=np.zeros((5, 4), np.float32), n_components=5),
                dict(x=np.zeros((5, 4), np.float32), n_components=0), dict(x=np.zeros((5, 200), np.float32), n_components=129),
                dict(x=np.zeros((5, 4), np.float32), n_sweeps=0), dict(x=np.zeros((5, 200), np.float32), n_iter=-1),
                dict(x=np.zeros((5, 200), np.float32), n_components=8, V0=np.zeros((200, 4))), dict(x=np.zeros(5, np.float32))):
        with pytest.raises(ValueError):
            pca.fit(**bad)
    with pytest.raises(ValueError):
        pca.eigh(np.zeros((129, 129)))
    with pytest.raises(ValueError):
        pca.eigh(np.zeros((3, 4)))
    assert pca.workspace_bytes(60000, 784, 58) > 784 * 784 * 8


def test_tsne_starts_from_the_principal_components():
    from gmvae_amd import pca, tsne
    x = torch.from_numpy(R.fixture(300, 12, decay=0.7, seed=71)).cuda()
    init = pca.tsne_init(x)
    f = pca.fit(x, n_components=2)
    sd = init.double().std(dim=0, unbiased=False)
    print(f"init: standard deviations {sd.tolist()}")
    assert init.shape == (300, 2) and abs(sd[0].item() / 1e-4 - 1.0) <= 1e-5
    assert abs(sd[1].item() / sd[0].item() - math.sqrt(f["explained_variance"][1].item() / f["explained_variance"][0].item())) <= 1e-5
    kw = dict(perplexity=20.0, n_iter=30, exaggeration_iters=20, seed=3)
    a, b = tsne.embed(x, init="pca", **kw), tsne.embed(x, init=init, **kw)
    assert torch.equal(a["embedding"], b["embedding"]) and torch.equal(a["kl_history"], b["kl_history"])
    none, again = tsne.embed(x, init=None, **kw), tsne.embed(x, **kw)              # the default is untouched: the Philox start of `seed`
    start = tsne.embed(x, init=tsne.initial_embedding(300, 3), **kw)
    assert torch.equal(none["embedding"], again["embedding"]) and torch.equal(none["embedding"], start["embedding"])
    assert not torch.equal(none["embedding"], a["embedding"])
    with pytest.raises(ValueError):
        tsne.embed(x, init="spectral", **kw)


def test_models_report_the_spectrum_of_their_codes():
    """model.latent_pca on test_linprobe.py's three small models: pca.fit of model.transform's codes plus the summary."""
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(3)
    x = torch.from_numpy((rng.random((64, 64)) < 0.5).astype(np.uint8)).cuda()
    for name, model in (("vae", create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)),
                        ("vae_gmp", create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)),
                        ("gmvae", create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1))):
        z = model.transform(x).cpu().numpy()
        o = model.latent_pca(x)
        print(f"{name}:")
        ref = R.fit(z)
        check_fit(o, ref)
        s = R.spectrum_summary(ref["explained_variance"], ref["total_variance"])
        assert o["dim90"].item() == s["dim90"]
        assert abs(o["participation"].item() - s["participation"]) <= 1e-9 * 4 and abs(o["top_ratio"].item() - s["top_ratio"]) <= 1e-9
        e = model.embed_latent(x, init="pca", perplexity=10.0, n_iter=5)
        assert e["embedding"].shape == (64, 2) and torch.isfinite(e["embedding"]).all().item()


def test_run_eval_reports_the_four_readouts(tmp_path):
    from gmvae_amd import pca, run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=300", "--batch_size=50"]
    run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--latent_pca=170", "--embed_latent=100", "--tsne_init=pca", "--tsne_perplexity=10", "--tsne_iters=10",
                          "--fit_latent_mixture=200", "--pca_baseline=6", "--sample_test=120", "--sample_test_space=code", "--sample_test_perms=20",
                          "--sample_frechet=120"] + args)
    keys = [f"train/{k}" for k in ("latent_pca_dim90", "latent_pca_participation", "latent_pca_top_ratio", "latent_pca_offdiag",
                                   "pca_mixture_loglik", "cluster_acc_pca_mixture", "pca_residual_max", "frechet_code")]
    for k in keys:
        assert k in res and math.isfinite(res[k]), k
    print({k: res[k] for k in keys})
    f = pca.fit(res["latent_state"][:170])
    for k in f:
        assert torch.equal(f[k], res["latent_pca"][k]), k
    assert res["train/latent_pca_offdiag"] <= K.GATE_OFFDIAG and 1 <= res["train/latent_pca_dim90"] <= 9
    assert res["latent_embedding"].shape == (100, 2)
    for flags in (["--tsne_init=pca"], ["--pca_baseline=4"], ["--pca_baseline=4", "--latent_pca=50"]):
        with pytest.raises(SystemExit):
            run_gmvae.main(["--mode=eval"] + flags + args)
