"""The statement of the linear probe (tests/linprobe_ref.py) against scikit-learn and against its own invariants, the data of the
device tests (tests/linprobe_cases.py), and the host-side argument checks of gmvae_linprobe_* (include/gmvae_hip.h) through ctypes:
no compute call, no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import linprobe_cases as K
import linprobe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gmvae_linprobe_workspace_bytes", "gmvae_linprobe_fit", "gmvae_linprobe_predict"}
E_NULL, E_DIMS, E_ALIGN = -1, -2, -4
P = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("shape", [(203, 5, 3), (1031, 64, 10)], ids=K.sid)
def test_statement_agrees_with_scikit_learn(shape):
    """300 iterations at l2 = 1e-2 against LogisticRegression (lbfgs, tol 1e-12) with C = 1 / (n l2): f - f* <= 1e-8, max |dW| <=
    1e-3 max |W|, the same argmax on every row, on overlapping clusters (linprobe_cases.overlapping).  Measured: f - f* = 1.0e-11 and
    3.8e-10, max |dW| = 1.3e-5 and 3.4e-5."""
    pytest.importorskip("sklearn")
    from sklearn.linear_model import LogisticRegression
    N, Lz, Cn = shape
    x, y = K.overlapping(shape)
    lab = R.labelled(y, Cn)
    n = int(lab.sum())
    assert 0.6 * N < n < 0.8 * N                      # 30 % of the rows are unlabelled
    f = R.fit(x, y, Cn, K.L2, 300)
    sk = LogisticRegression(C=1.0 / (n * K.L2), tol=1e-12, max_iter=20000, fit_intercept=True).fit(x[lab].astype(np.float64), y[lab])
    assert list(sk.classes_) == list(range(Cn))
    W_sk, b_sk = sk.coef_.T, sk.intercept_
    f_ours, f_star = R.objective(x, y, Cn, K.L2, f["W"], f["b"]), R.objective(x, y, Cn, K.L2, W_sk, b_sk)
    dW = np.abs(f["W"] - W_sk).max()
    print(f"{shape}: f - f* = {f_ours - f_star:.3e}, max|dW| = {dW:.3e}, max|W| = {np.abs(W_sk).max():.3e}")
    assert f_ours - f_star <= 1e-8
    assert dW <= 1e-3 * np.abs(W_sk).max()
    ours = R.predict(x, f["W"], f["b"])["pred"]
    theirs = (x.astype(np.float64) @ W_sk + b_sk).argmax(axis=1)
    assert (ours == theirs).all()


@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_statement_invariants(shape):
    """loss_history[0] = ln C; the columns of W and b sum to 0; f(Theta_it) stays under f(0); the un-centred (W, b) reproduce the
    centred logits; permuting the unlabelled rows' codes changes nothing."""
    N, Lz, Cn = shape
    x, y = K.data(shape)
    f = R.fit(x, y, Cn, K.L2, 50, theta_history=True)
    assert f["info"] == 0
    assert abs(f["loss_history"][0] - math.log(Cn)) <= 1e-12
    assert np.abs(f["W"].sum(axis=1)).max() <= 1e-10 and abs(f["b_centred"].sum()) <= 1e-10
    f0 = math.log(Cn)
    for ThW, Thb in f["thetas"]:
        assert R.objective(x, y, Cn, K.L2, ThW, Thb, xbar=f["xbar"]) <= f0
    x64 = x.astype(np.float64)
    centred, plain = (x64 - f["xbar"]) @ f["W"] + f["b_centred"], x64 @ f["W"] + f["b"]
    assert np.abs(centred - plain).max() <= 1e-10 * max(1.0, np.abs(centred).max())
    lab = R.labelled(y, Cn)
    if (~lab).sum() >= 2:
        xp = x.copy()
        rows = np.flatnonzero(~lab)
        xp[rows] = x[np.roll(rows, 1)]
        g = R.fit(xp, y, Cn, K.L2, 50)
        assert np.array_equal(g["W"], f["W"]) and np.array_equal(g["b"], f["b"]) and np.array_equal(g["loss_history"], f["loss_history"])


def test_fp32_exponentials_move_the_fit_by_rounding_only():
    """The device's fp32 exponentials: W after 300 iterations moves by <= 1e-6 max |W| (measured 2e-8 absolute): the scheme does
    not amplify rounding, and the device tests' 1e-4 gate is four orders wider."""
    shape = (1031, 64, 10)
    x, y = K.data(shape)
    a, b = R.fit(x, y, 10, K.L2, 300), R.fit(x, y, 10, K.L2, 300, exp_dtype=np.float32)
    d = np.abs(a["W"] - b["W"]).max()
    print(f"max|dW| = {d:.3e}, max|W| = {np.abs(a['W']).max():.3e}")
    assert d <= 1e-6 * np.abs(a["W"]).max()


@pytest.mark.parametrize("n_iter", K.ITERS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_device_cases_leave_no_row_out_of_the_argmax_check(shape, n_iter):
    """tests/test_linprobe.py compares pred where the reference's top two log-probs differ by more than 1e-4 and allows 1 % of the rows
    to be left out: in its cases no row is, but for C = 256 after ONE iteration -- the logits of that point are of the order 1 / C
    whatever the separation of the clusters (the first step is invariant to the scale of the codes), and 13 of the 4,099 rows
    (0.32 %) have their two best classes within 1e-4."""
    lp = K.reference(shape, n_iter)["predict"]["log_prob"]
    m = K.margins(lp)
    out = int((m <= K.MARGIN).sum())
    print(f"{shape} after {n_iter}: the smallest margin {m.min():.3e}, {out} rows left out")
    assert out <= 0.01 * shape[0]
    assert out == (13 if (shape, n_iter) == ((4099, 16, 256), 1) else 0)


def test_failures_of_the_set_up():
    x, y = K.data((203, 5, 3))
    none = R.fit(x, np.full(203, -1), 3, K.L2, 4)
    assert none["info"] == -1 and not none["W"].any() and np.isnan(none["loss_history"]).all() and math.isnan(none["grad_max"])
    chol, info = R.cholesky_info(np.diag([1.0, -1.0, 1.0]))
    assert chol is None and info == 2
    zero = R.fit(x, y, 3, K.L2, 0)
    assert zero["info"] == 0 and not zero["W"].any() and zero["loss_history"].shape == (0,) and math.isnan(zero["grad_max"])
    assert R.betas(3)[0] == 0.0 and abs(R.betas(3)[1] - (0.5 * (1 + math.sqrt(5)) - 1) / (0.5 * (1 + math.sqrt(1 + (1 + math.sqrt(5)) ** 2)))) < 1e-15


# ------------------------------------------------------------------------------------------------------------ the host side
def test_names_are_declared_exported_and_bound(L):
    hdr = open(os.path.join(ROOT, "include", "gmvae_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\bint\s+(\w+)\s*\(", hdr))
    assert NAMES <= declared <= set(L.EXPORTS)
    raw = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and getattr(L.lib, name).argtypes is not None
    assert L.lib.gmvae_abi_version() == L.ABI_VERSION == 7


def size(L, N, Lz, Cn):
    b = C.c_uint64()
    return L.lib.gmvae_linprobe_workspace_bytes(N, Lz, Cn, C.byref(b)), b.value


def groups(N, T):
    """csrc/mixfit_common.hpp mf_plan_groups: N rows in tiles of T, whole tiles per workgroup, 256 workgroups at most."""
    tiles = -(-N // T)
    per = -(-tiles // min(tiles, 256)) * T
    return -(-N // per)


def plan(N, Lz, Cn):
    """csrc/linprobe.hpp lp_plan: (workspace bytes, the pass's workgroups G and rows per tile T, the set-up's workgroups Gs)."""
    Lp, Cp, P = Lz | 1, Cn | 1, Lz * (Lz + 1) // 2
    image, row = 8 * Cn + 4 * Lz * Cn, 8 * (Cp + 4) + 4 * (Lp + 2)
    T = min(128, (163840 - image) // row, N)
    G, Gs = groups(N, T), groups(N, 64)
    doubles = 4 + Lz + Lz * Lz + 2 * Cn * (Lz + 1) + 2 * Cn + max(G * (Cn * (Lz + 1) + 3), Gs * (P + Lz + 1))
    return -(-8 * doubles // 16) * 16, G, T, Gs


# the gate: 1 <= N <= 2^24, 1 <= L <= 128, 2 <= C <= 256, C L <= 16,384
BAD_SIZES = [(0, 4, 3), (-5, 4, 3), ((1 << 24) + 1, 4, 3), (64, 0, 3), (64, 129, 2), (64, 4, 1), (64, 4, 0), (64, 4, 257),
             (64, 65, 253), (64, 128, 129)]


def test_workspace_size_follows_the_plan(L):
    for shape in K.SHAPES + [(60000, 64, 10), (1 << 24, 128, 128), (1 << 24, 64, 256), (1 << 24, 1, 2), (5, 128, 128)]:
        rc, b = size(L, *shape)
        want, G, T, Gs = plan(*shape)
        assert rc == 0 and b == want and b % 16 == 0, (shape, b, want)
        assert 1 <= G <= 256 and 1 <= T <= 128 and 1 <= Gs <= 256
        N, Lz, Cn = shape
        # the LDS of the pass, of linprobe_gram (64 rows a tile) and of linprobe_setup fits the 160 KiB of a CU
        assert 8 * (Cn + T * ((Cn | 1) + 4)) + 4 * (Lz * Cn + T * ((Lz | 1) + 2)) <= 163840
        assert 8 * (Lz * (Lz + 1) // 2 + 64 * (Lz | 1) + Lz + 1) <= 163840 and 8 * (Lz * (Lz + 1) + Lz + 1) <= 163840
    assert size(L, 64, 64, 256)[0] == 0 and size(L, 64, 128, 128)[0] == 0                  # C L = 16,384 is inside the gate
    assert size(L, 64, 65, 253)[0] == E_DIMS                                               # 16,445 is not; nor is 16,385 = 5 x 29 x 113:
    assert 113 * 145 == 16385 and size(L, 64, 113, 145)[0] == E_DIMS
    for bad in BAD_SIZES:
        assert size(L, *bad)[0] == E_DIMS, bad
    assert L.lib.gmvae_linprobe_workspace_bytes(8, 8, 2, None) == E_NULL
    assert L.lib.gmvae_linprobe_workspace_bytes(0, 8, 2, None) == E_DIMS                   # the sizes come first
    from gmvae_amd import linprobe
    assert linprobe.workspace_bytes(1031, 64, 10) == plan(1031, 64, 10)[0]


def _p(a):
    return None if a is None else C.c_void_p(a)


def fit(L, codes=P, labels=P, N=64, Lz=4, Cn=3, l2=1e-3, n_iter=3, W=P, b=P, hist=P, gmax=P, info=P, ws=P):
    return L.lib.gmvae_linprobe_fit(_p(codes), _p(labels), N, Lz, Cn, l2, n_iter, _p(W), _p(b), _p(hist), _p(gmax), _p(info), _p(ws), None)


def predict(L, codes=P, labels=P, N=64, Lz=4, Cn=3, W=P, b=P, log_prob=P, pred=P, sums=P, ws=P):
    return L.lib.gmvae_linprobe_predict(_p(codes), _p(labels), N, Lz, Cn, _p(W), _p(b), _p(log_prob), _p(pred), _p(sums), _p(ws), None)


def test_every_failing_argument_returns_its_documented_code(L):
    for fn, ptrs, optional in ((fit, ("codes", "labels", "W", "b", "ws"), ("hist", "gmax", "info")),
                               (predict, ("codes", "W", "b", "ws"), ("labels", "log_prob", "pred", "sums"))):
        f = lambda **kw: fn(L, **kw)
        for N, Lz, Cn in BAD_SIZES + [(64, 113, 145)]:
            assert f(N=N, Lz=Lz, Cn=Cn) == E_DIMS, (fn.__name__, N, Lz, Cn)
        for name in ptrs:
            assert f(**{name: None}) == E_NULL, (fn.__name__, name)
            assert f(**{name: None}, N=0) == E_DIMS, (fn.__name__, name)                       # the sizes come first,
            other = ptrs[0] if name != ptrs[0] else ptrs[1]
            assert f(**{name: None, other: P + 2}) == E_NULL, (fn.__name__, name)              # then NULL, then the alignment
            assert f(**{name: P + (8 if name == "ws" else 2)}) == E_ALIGN, (fn.__name__, name)
        for name in optional:
            assert f(**{name: P + (4 if name == "sums" else 2)}) == E_ALIGN, (fn.__name__, name)
            assert f(**{name: None, "codes": None}) == E_NULL, (fn.__name__, name)             # (NULL there is no error of its own)
    for l2 in (0.0, -1e-3, float("nan"), float("inf")):
        assert fit(L, l2=l2) == E_DIMS and fit(L, l2=l2, codes=None) == E_DIMS, l2
    assert fit(L, n_iter=-1) == E_DIMS and fit(L, n_iter=-1, codes=None) == E_DIMS
    # the gate's edges pass the size check (and fail the next one)
    assert fit(L, Lz=128, Cn=128, codes=None) == E_NULL and fit(L, Lz=64, Cn=256, codes=None) == E_NULL
    assert fit(L, Lz=1, Cn=2, N=1, codes=None) == E_NULL and predict(L, Lz=128, Cn=2, N=1 << 24, codes=None) == E_NULL


def test_python_gate_raises_value_errors(L, monkeypatch):
    """gmvae_amd.linprobe refuses what the library would, as ValueError, before it asks for a device."""
    import torch
    from gmvae_amd import linprobe
    monkeypatch.setattr(linprobe, "_codes", lambda c: torch.as_tensor(c, dtype=torch.float32))
    y = torch.zeros(8, dtype=torch.int32)
    for Lz, Cn in ((129, 2), (4, 1), (4, 257), (113, 145)):
        with pytest.raises(ValueError):
            linprobe.fit(torch.zeros(8, Lz), y, Cn)
    for kw in ({"l2": 0.0}, {"l2": float("nan")}, {"n_iter": -1}):
        with pytest.raises(ValueError):
            linprobe.fit(torch.zeros(8, 4), y, 3, **kw)
    with pytest.raises(ValueError):
        linprobe.fit(torch.zeros(8, 4), torch.full((8,), -1), 3)                               # no labelled row, seen on the host
    with pytest.raises(ValueError):
        linprobe.fit(torch.zeros(8, 4), torch.zeros(7, dtype=torch.int32), 3)


def test_runner_flag_checks(L, monkeypatch):
    from gmvae_amd import run_gmvae
    p = run_gmvae.build_parser()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ok = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--linear_probe=64", "--probe_test=32", "--probe_l2=0.01", "--probe_iters=10",
                                               "--probe_labelled_per_class=5", "--probe_standardize"]))
    assert (ok.linear_probe, ok.probe_test, ok.probe_l2, ok.probe_iters, ok.probe_labelled_per_class, ok.probe_standardize) == \
        (64, 32, 0.01, 10, 5, True)
    plain = run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--linear_probe=64"]))
    assert (plain.probe_test, plain.probe_l2, plain.probe_iters) == (0, 1e-3, 300)
    for bad in (["--mode=train", "--linear_probe=64"], ["--mode=eval", "--linear_probe=-1"], ["--mode=eval", "--probe_iters=10"],
                ["--mode=eval", "--linear_probe=64", "--probe_l2=0"], ["--mode=eval", "--linear_probe=64", "--latent_size=129"]):
        with pytest.raises(SystemExit):
            run_gmvae.check_args(p, p.parse_args(bad))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        run_gmvae.check_args(p, p.parse_args(["--mode=eval", "--linear_probe=64"]))
