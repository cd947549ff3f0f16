"""gmvae_linprobe_* (include/gmvae_hip.h; csrc/linprobe.hpp) and gmvae_amd.linprobe on the device against the fp64 statement
(tests/linprobe_ref.py): the fit after 1 and after 50 iterations and the prediction of the fitted probe on six shapes
(tests/linprobe_cases.py); labels out of range and a class without a labelled row; saturated logits; a constant code column; a
fit without a labelled row; bit-equality of two runs; fit and predict in stream order; the Python, model and runner surface.

Gate (the project's own, for gradients and for mixfit's log r): every output tensor -- W, b, loss_history, log_prob -- within 1e-4 of
its OWN maximum magnitude in the reference (a tensor that is 0 in the reference is 0 on the device).  pred equals the reference's
argmax wherever the reference's two best log-probs differ by more than 1e-4, and at most 1 % of the rows are left out by that rule
(tests/test_linprobe_cpu.py: none, but 13 of 4,099 for C = 256 after one iteration).  Every test prints its worst figure before it
asserts."""
import math

import numpy as np
import pytest
import torch

import linprobe_cases as K
import linprobe_ref as R

pytestmark = pytest.mark.gpu


def gate(name, got, ref):
    """The worst |got - ref| of a tensor in units of the gate, 1e-4 max |ref|; printed, then asserted <= 1."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), name
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"  {name}: max |got - ref| = {err:.3e}, max |ref| = {top:.3e}")
    assert err <= K.GATE * top, (name, err, top)


def check_fit(got, ref):
    assert int(got["info"].item()) == ref["info"] == 0
    gate("W", got["W"].cpu().numpy(), ref["W"])
    gate("b", got["b"].cpu().numpy(), ref["b"])
    gate("loss_history", got["loss_history"].cpu().numpy(), ref["loss_history"])


def check_predict(x, y, got_fit, ref, C):
    """The device's prediction of the DEVICE's probe against the reference's prediction of the reference's probe."""
    from gmvae_amd import linprobe
    sc = linprobe.score(x, y, got_fit)
    rp = ref["predict"] if "predict" in ref else R.predict(x, ref["W"], ref["b"], y, C)
    gate("log_prob", sc["log_prob"].cpu().numpy(), rp["log_prob"])
    m = K.margins(rp["log_prob"])
    keep = m > K.MARGIN
    print(f"  pred: {int((~keep).sum())} of {len(m)} rows left out, the smallest margin {m.min():.3e}")
    assert (~keep).sum() <= 0.01 * len(m)
    pred = sc["pred"].cpu().numpy()
    assert pred.dtype == np.int32 and (pred[keep] == rp["pred"][keep]).all()
    n, hits, nll = rp["sums"]
    assert sc["n"].item() == n
    if keep.all():
        assert round(sc["accuracy"].item() * n) == hits
    if n:
        top = np.abs(rp["log_prob"]).max()
        print(f"  nll: |got - ref| = {abs(sc['nll'].item() - nll / n):.3e}")
        assert abs(sc["nll"].item() - nll / n) <= K.GATE * top
    return sc


@pytest.mark.parametrize("n_iter", K.ITERS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.sid)
def test_fit_and_predict_match_the_statement(shape, n_iter):
    from gmvae_amd import linprobe
    x, y = K.data(shape)
    ref = K.reference(shape, n_iter)
    got = linprobe.fit(x, y, shape[2], l2=K.L2, n_iter=n_iter)
    print(f"{shape} after {n_iter}:")
    check_fit(got, ref)
    # the gradient's own maximum magnitude is the one it starts from
    g0 = K.reference(shape, 1)["grad_max"]
    print(f"  grad_max: got {got['grad_max'].item():.6e}, ref {ref['grad_max']:.6e}")
    assert abs(got["grad_max"].item() - ref["grad_max"]) <= K.GATE * g0
    check_predict(x, y, got, ref, shape[2])


def test_labels_out_of_range_and_a_class_without_a_labelled_row():
    """-1, C and -7 all mark a row unlabelled; class 2 of 5 has no labelled row: its column of W follows the penalty and the
    other classes' probabilities alone."""
    from gmvae_amd import linprobe
    N, Lz, C = 389, 11, 5
    x, _, y_true = R.clusters(N, Lz, C, seed=31, sep=4.0, unlabelled=0.0)
    y = y_true.copy()
    y[y_true == 2] = np.array([-1, C, -7])[np.arange((y_true == 2).sum()) % 3]
    y[::7] = np.array([C, -7, -1, 1000, -2 ** 31])[np.arange(len(y[::7])) % 5]
    assert not (y == 2).any() and R.labelled(y, C).sum() > 200
    for n_iter in (1, 50):
        ref = R.fit(x, y, C, K.L2, n_iter)
        got = linprobe.fit(x, y, C, l2=K.L2, n_iter=n_iter)
        print(f"labels after {n_iter}:")
        check_fit(got, ref)
        check_predict(x, y, got, ref, C)
    every = linprobe.score(x, y_true, got)                    # scored on the true labels: the rows of class 2 count, and are all wrong
    rp = R.predict(x, ref["W"], ref["b"], y_true, C)
    assert every["n"].item() == N and round(every["accuracy"].item() * N) == rp["sums"][1]
    none = linprobe.predict(x, got)
    assert set(none) == {"log_prob", "pred"} and torch.equal(none["pred"], every["pred"]) and torch.equal(none["log_prob"], every["log_prob"])


def test_saturated_logits_stay_finite():
    """Separable codes scaled by 1e3 with l2 = 1e-6: the fit against the statement under the same gate; then the same probe with W and
    b scaled until the logits reach 1e4: log_prob is finite and within the gate."""
    from gmvae_amd import linprobe
    x, y, C = K.saturated()
    for n_iter in (1, 50):
        ref = R.fit(x, y, C, 1e-6, n_iter)
        got = linprobe.fit(x, y, C, l2=1e-6, n_iter=n_iter)
        print(f"saturated after {n_iter}:")
        check_fit(got, ref)
        check_predict(x, y, got, ref, C)
    W, b = got["W"].cpu().numpy(), got["b"].cpu().numpy()
    reach = np.abs(x.astype(np.float64) @ W + b).max()
    s = np.float32(2e4 / reach)
    Ws, bs = (W * s).astype(np.float32), (b * s).astype(np.float32)
    rp = R.predict(x, Ws, bs, y, C)
    assert np.abs(x.astype(np.float64) @ Ws + bs).max() >= 1e4
    sc = linprobe.score(x, y, (torch.from_numpy(Ws), torch.from_numpy(bs)))
    lp = sc["log_prob"].cpu().numpy()
    gate("log_prob at logits of 1e4", lp, rp["log_prob"])
    assert math.isfinite(sc["nll"].item())
    keep = K.margins(rp["log_prob"]) > K.MARGIN
    assert (~keep).sum() <= 0.01 * len(keep) and (sc["pred"].cpu().numpy()[keep] == rp["pred"][keep]).all()


def test_a_constant_code_column():
    """Column 3 is 2.5 in every row: its centred values are exactly 0, A is positive definite through l2 alone in that direction, and
    row 3 of the statement's W stays 0 (the device centres the SUMS, sum x r - xbar sum r, and is there at rounding: inside the gate
    on W)."""
    from gmvae_amd import linprobe
    x, y, _ = R.clusters(211, 6, 3, seed=41, sep=4.0)
    x[:, 3] = 2.5
    ref = R.fit(x, y, 3, K.L2, 50)
    got = linprobe.fit(x, y, 3, l2=K.L2, n_iter=50)
    check_fit(got, ref)
    assert not ref["W"][3].any()
    print(f"  row 3 of W on the device: {got['W'][3].abs().max().item():.3e}")
    check_predict(x, y, got, ref, 3)


def test_no_labelled_row_and_no_iteration():
    from gmvae_amd import linprobe
    x, y = K.data((203, 5, 3))
    dev_labels = torch.full((203,), -1, dtype=torch.int32, device="cuda")      # on the device: not read back, so reported in info
    got = linprobe.fit(x, dev_labels, 3, n_iter=4)
    assert got["info"].item() == -1 and not got["W"].any().item() and not got["b"].any().item()
    assert torch.isnan(got["loss_history"]).all().item() and math.isnan(got["grad_max"].item())
    zero = linprobe.fit(x, y, 3, n_iter=0)
    assert zero["info"].item() == 0 and not zero["W"].any().item() and zero["loss_history"].shape == (0,)
    assert math.isnan(zero["grad_max"].item())
    sc = linprobe.score(x, y, zero)                        # W = b = 0: every class at ln 1/3, pred the first index
    assert not sc["pred"].any().item() and abs(sc["nll"].item() - math.log(3)) <= 1e-6


def test_two_runs_give_the_same_bits_and_fit_and_predict_follow_the_stream():
    from gmvae_amd import linprobe
    shape = (1031, 64, 10)
    x, y = K.data(shape)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    a = linprobe.fit(xd, yd, 10, l2=K.L2, n_iter=50)
    pa = linprobe.score(xd, yd, a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # fit, then predict, enqueued on one stream with nothing in between
        b = linprobe.fit(xd, yd, 10, l2=K.L2, n_iter=50)
        pb = linprobe.score(xd, yd, b)
    side.synchronize()
    for k in ("W", "b", "loss_history", "grad_max", "info"):
        assert torch.equal(a[k], b[k]), k
    for k in ("log_prob", "pred", "accuracy", "nll", "n"):
        assert torch.equal(pa[k], pb[k]), k
    check_fit(b, K.reference(shape, 50))


def test_standardize():
    """standardize=True is the fit of the codes centred and scaled by the labelled rows' mean and standard deviation (fp64), and
    predict and score apply the same map."""
    from gmvae_amd import linprobe
    x, y, _ = R.clusters(307, 9, 4, seed=51, sep=3.0)
    x = (x * np.linspace(0.1, 30.0, 9) + 5.0).astype(np.float32)
    lab = R.labelled(y, 4)
    mean, sd = x[lab].astype(np.float64).mean(axis=0), x[lab].astype(np.float64).std(axis=0)
    xs = ((x.astype(np.float64) - mean) / sd).astype(np.float32)
    got = linprobe.fit(x, y, 4, l2=K.L2, n_iter=50, standardize=True)
    assert np.abs(got["mean"].cpu().numpy() - mean).max() <= 1e-12 * 40 and np.abs(got["scale"].cpu().numpy() - sd).max() <= 1e-12 * 40
    ref = R.fit(xs, y, 4, K.L2, 50)
    check_fit(got, ref)
    sc = linprobe.score(x, y, got)
    gate("log_prob", sc["log_prob"].cpu().numpy(), R.predict(xs, ref["W"], ref["b"])["log_prob"])


def test_models_probe_their_codes():
    """model.linear_probe on a small VAE, mixture-prior VAE and GMVAE with B = 64: the fit of linprobe.fit on model.transform's codes;
    labelled_per_class shows the fit the rows runners.select_labelled picks."""
    from gmvae_amd import linprobe, runners
    from gmvae_amd.gmvae import create_gmvae
    from gmvae_amd.vae import create_vae
    rng = np.random.default_rng(3)
    x = torch.from_numpy((rng.random((64, 64)) < 0.5).astype(np.uint8)).cuda()
    xt = torch.from_numpy((rng.random((64, 64)) < 0.5).astype(np.uint8)).cuda()
    labels, test_labels = torch.from_numpy(rng.integers(0, 4, 64)), torch.from_numpy(rng.integers(0, 4, 64))
    for name, model in (("vae", create_vae(64, 4, fcnet_hidden_sizes=[16], random_seed=1)),
                        ("vae_gmp", create_vae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1)),
                        ("gmvae", create_gmvae(64, 4, mixture_components=3, fcnet_hidden_sizes=[16], random_seed=1))):
        z, zt = model.transform(x).cpu().numpy(), model.transform(xt).cpu().numpy()
        o = model.linear_probe(x, labels, xt, test_labels, n_classes=4, l2=K.L2, n_iter=20)
        assert set(o) == {"fit", "train_accuracy", "train_nll", "n_labelled", "test_accuracy", "test_nll"}, name
        ref = R.fit(z, labels.numpy(), 4, K.L2, 20)
        print(f"{name}:")
        check_fit(o["fit"], ref)
        tr, te = R.predict(z, ref["W"], ref["b"], labels.numpy()), R.predict(zt, ref["W"], ref["b"], test_labels.numpy())
        assert o["n_labelled"].item() == 64
        assert abs(o["train_nll"].item() - tr["sums"][2] / 64) <= 1e-4 * np.abs(tr["log_prob"]).max()
        assert abs(o["test_nll"].item() - te["sums"][2] / 64) <= 1e-4 * np.abs(te["log_prob"]).max()
        assert round(o["train_accuracy"].item() * 64) == tr["sums"][1] or (K.margins(tr["log_prob"]) <= K.MARGIN).any()
        assert 0.0 <= o["test_accuracy"].item() <= 1.0
        few = model.linear_probe(x, labels, n_classes=4, labelled_per_class=3, seed=5, l2=K.L2, n_iter=20)
        shown = runners.select_labelled(labels.numpy(), 3, 5)
        assert set(few) == {"fit", "train_accuracy", "train_nll", "n_labelled"} and few["n_labelled"].item() == (shown >= 0).sum() == 12
        check_fit(few["fit"], R.fit(z, shown, 4, K.L2, 20))
    with pytest.raises(ValueError):
        model.linear_probe(x, labels, xt, n_classes=4)
    assert linprobe.workspace_bytes(64, 4, 4) > 0


def test_run_eval_reports_the_linear_probe(tmp_path):
    from gmvae_amd import linprobe, run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--max_steps=20", "--summarise_every=10", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=300", "--batch_size=50"]
    run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--linear_probe=170", "--probe_test=90", "--probe_iters=30", "--probe_l2=0.01"] + args)
    keys = [f"train/linear_probe_{k}" for k in ("acc", "nll", "train_acc", "grad_max")]
    for k in keys:
        assert k in res and math.isfinite(res[k]), k
    codes, labs = res["latent_state"], res["labels"]
    fitted = linprobe.fit(codes[:170], labs[:170], 10, l2=0.01, n_iter=30)
    assert torch.equal(fitted["W"], res["linear_probe"]["W"]) and torch.equal(fitted["b"], res["linear_probe"]["b"])
    te = linprobe.score(codes[170:260], labs[170:260], fitted)
    assert res["train/linear_probe_acc"] == te["accuracy"].item() and res["train/linear_probe_nll"] == te["nll"].item()
    ref = R.fit(codes[:170].cpu().numpy(), labs[:170].cpu().numpy(), 10, 0.01, 30)
    check_fit(fitted, ref)
    # --probe_test defaults to what is left, N at most; the M1 baseline and the standardised probe report the same keys
    res = run_gmvae.main(["--mode=eval", "--linear_probe=200", "--probe_iters=5", "--probe_labelled_per_class=2", "--probe_standardize"] + args)
    for k in keys:
        assert k in res and math.isfinite(res[k]), k
    assert set(res["linear_probe"]) >= {"W", "b", "mean", "scale"}
    with pytest.raises(ValueError):
        run_gmvae.main(["--mode=eval", "--linear_probe=300"] + args)                           # nothing left to score
