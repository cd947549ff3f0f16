"""gmvae_impute on the device through the C ABI against the fp64 statement (tests/impute_ref.py) on the regenerated noise, at the
cases of tests/impute_cases.py: the log weights at the project's row gate, the mean image with the fold isolated from the weights'
sensitivity and against the pure statement within the exact bound of a self-normalised sum, the stats, the draws, the invariances,
the all-ones mask, the refusals, and the model / runner API.  x is flipped at the missing pixels: any use of x there shows."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import impute_cases as IC
import impute_ref as IR
import pmask_ref as PR
from hip_util import _L, dev, dims_of, write_inputs

pytestmark = pytest.mark.gpu

SEED, STEP, M = IC.SEED, IC.STEP, IC.M_DRAWS
_RUNS = {}


def _cdims(d, B, chunk, bit=True, row0=0, extra=0):
    cd = dims_of(dataclasses.replace(d, S=chunk), B)
    cd.sched_flags = (_L().OBJ_PIXEL_MASK if bit else 0) | extra
    cd.row0 = row0
    return cd


def impute(model, d, flat, x, mask, n, chunk, n_draws=M, bit=True, row0=0):
    """One gmvae_impute call (slot 0 of the masks = mask when the dims carry the bit): dict of numpy outputs, each NaN (-1 for
    the indices) until the call writes it."""
    import torch
    L = _L()
    B = x.shape[0]
    cd = _cdims(d, B, chunk, bit, row0)
    ws = torch.zeros(L.impute_workspace_bytes(cd, model, n_draws) // 4 + 64, dtype=torch.float32, device="cuda")
    if bit:
        write_inputs(ws, cd, model, {"pixel_mask": mask})
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    o = dict(mean=nan(B, d.D), stats=nan(B, 4), logw=nan(B, n), tail=nan(L.TAIL),
             draw_index=torch.full((B, max(n_draws, 1)), -1, dtype=torch.int64, device="cuda"), draw_z=nan(B, max(n_draws, 1), d.L))
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    L.check(L.lib.gmvae_impute(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, n_draws, L.ptr(o["mean"]), L.ptr(o["stats"]),
                               L.ptr(o["logw"]), L.ptr(o["draw_index"]) if n_draws else None,
                               L.ptr(o["draw_z"]) if n_draws else None, L.ptr(o["tail"]), L.ptr(ws), SEED, STEP, L.current_stream()),
            "gmvae_impute")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def run(name, n, chunk):
    """The case's device run with its own mask and the flipped x: once, shared, left unchanged."""
    if (name, n, chunk) not in _RUNS:
        model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
        _RUNS[name, n, chunk] = impute(model, d, flat, xf, m, n, chunk)
    return _RUNS[name, n, chunk]


def _g(logw, ref):
    """g_b = max_s |log w_bs - ref_bs|."""
    return np.abs(logw.astype(np.float64) - ref).max(axis=1)


def _iw_bound(model, d, flat, x, mask, n, chunk):
    import torch
    L = _L()
    B = x.shape[0]
    cd = _cdims(d, B, chunk)
    ws = torch.zeros(L.iw_bound_workspace_bytes(cd, model) // 4 + 64, dtype=torch.float32, device="cuda")
    write_inputs(ws, cd, model, {"pixel_mask": mask})
    bound, tail = torch.full((B,), float("nan"), device="cuda"), torch.full((L.TAIL,), float("nan"), device="cuda")
    params, xd = dev(flat, torch.float32), dev(x, torch.uint8)
    L.check(L.lib.gmvae_iw_bound(C.byref(cd), model, L.ptr(xd), L.ptr(params), n, L.ptr(bound), None, L.ptr(tail), L.ptr(ws),
                                 SEED, STEP, L.current_stream()), "gmvae_iw_bound")
    torch.cuda.synchronize()
    return bound.cpu().numpy()


# 1 - 5 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,chunk", IC.PARAMS)
def test_outputs_match_the_statement(name, n, chunk):
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
    B = x.shape[0]
    s, e = IC.statement(name, n)
    o = run(name, n, chunk)
    lw_ref = s["lw"]
    # 1: the log weights at the row gate, and g_b at 1e-5 of the row's scale
    g = _g(o["logw"], lw_ref)
    scale = np.maximum(np.abs(lw_ref).max(axis=1), 1.0)
    print(f"{name} n={n} chunk={chunk}: g_b max {g.max():.3e} (relative {np.max(g / scale):.3e})")
    assert (np.abs(o["logw"] - lw_ref) <= 1e-4 * np.maximum(np.abs(lw_ref), 1.0)).all()
    assert (g <= 1e-5 * scale).all(), (g, scale)
    # 2: the fold alone: the statement on the DEVICE's log w and the reference's logits
    on_dev = IR.estimate(o["logw"].astype(np.float64), s["lam"], s["hid"])
    err_fold = np.abs(o["mean"] - on_dev["mean"]).max()
    # 3: the pure statement, within the exact bound of a self-normalised sum whose log weights moved by at most g_b
    err_pure = np.abs(o["mean"] - e["mean"]).max(axis=1)
    print(f"  mean: fold error {err_fold:.3e} (gate {IC.MEAN_GATE:.3e}); against the pure statement {err_pure.max():.3e}")
    assert np.isfinite(o["mean"]).all() and err_fold <= IC.MEAN_GATE
    assert (err_pure <= IR.weight_bound(g) + IC.MEAN_GATE).all()
    # 4: the stats and the tail
    st = o["stats"]
    assert np.array_equal(st[:, 0], _iw_bound(model, d, flat, xf, m, n, chunk))
    assert (np.abs(st[:, 0] - e["bound"]) <= 1e-4 * np.maximum(np.abs(e["bound"]), 1.0)).all()
    rel = 1e-4 + IR.weight_bound(g)
    print(f"  ess error {np.max(np.abs(st[:, 1] - e['ess']) / e['ess']):.3e} max weight error "
          f"{np.max(np.abs(st[:, 3] - e['max_weight']) / e['max_weight']):.3e} cond error {np.max(np.abs(st[:, 2] - e['cond'])):.3e}")
    assert (np.abs(st[:, 1] - e["ess"]) <= rel * e["ess"]).all()
    assert (np.abs(st[:, 3] - e["max_weight"]) <= rel * e["max_weight"]).all()
    assert (np.abs(st[:, 2] - e["cond"]) <= 1e-4 * np.maximum(np.abs(e["cond"]), 1.0) + 2 * g).all()
    t = o["tail"]
    assert t[3] == float((m == 0).sum()) and t[4] == B and (t[5:] == 0).all()
    assert abs(t[0] + st[:, 0].astype(np.float64).sum()) <= 1e-5 * abs(t[0])
    assert abs(t[1] - st[:, 1].astype(np.float64).sum()) <= 1e-5 * abs(t[1])
    assert abs(t[2] - st[:, 2].astype(np.float64).sum()) <= 1e-5 * abs(t[2])
    # 5: sampling-importance-resampling: the draws whose two best keys are far enough apart to compare
    cmpd = IR.compared_draws(lw_ref, e["key_gap"])
    assert 1.0 - cmpd.mean() <= IC.MAX_LEFT_OUT
    assert ((o["draw_index"] >= 0) & (o["draw_index"] < n)).all()
    assert np.array_equal(o["draw_index"][cmpd], e["draw_index"][cmpd])
    zr = np.take_along_axis(s["z"], o["draw_index"][:, :, None], axis=1)
    assert (np.abs(o["draw_z"] - zr) <= 1e-5 * np.maximum(np.abs(zr), 1.0))[cmpd].all()


# 6 --------------------------------------------------------------------------------------------------------------
_OUTS = ("mean", "stats", "logw", "tail", "draw_index", "draw_z")


@pytest.mark.parametrize("name,n,chunk", [("gumbel-784", 40, 16), ("vae-saturated", 7, 3)])
def test_two_calls_give_the_same_bits(name, n, chunk):
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
    a, b = run(name, n, chunk), impute(model, d, flat, xf, m, n, chunk)
    for k in _OUTS:
        assert np.array_equal(a[k], b[k]), k


def _within_weight_bound(a, b, what):
    g = _g(a["logw"], b["logw"].astype(np.float64))
    err = np.abs(a["mean"] - b["mean"]).max(axis=1)
    print(f"{what}: g {g.max():.3e} mean difference {err.max():.3e} bit-equal {np.array_equal(a['mean'], b['mean'])}")
    assert (err <= IR.weight_bound(g) + IC.MEAN_GATE).all()
    assert (np.abs(a["stats"][:, 0] - b["stats"][:, 0]) <= 1e-5 * np.maximum(np.abs(a["stats"][:, 0]), 1.0)).all()


def test_rows_one_at_a_time():
    """Rows of a B = 8 call against the same rows run one at a time with row0 = b."""
    name, n, chunk = "gumbel", 7, 3
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
    whole = run(name, n, chunk)
    assert xf.shape[0] == 8
    rows = [impute(model, d, flat, xf[b:b + 1], m[b:b + 1], n, chunk, row0=b) for b in range(8)]
    one = {k: np.concatenate([r[k] for r in rows]) for k in ("mean", "stats", "logw", "draw_index", "draw_z")}
    _within_weight_bound(whole, one, "B = 8 against one row at a time")
    assert np.array_equal(whole["draw_index"], one["draw_index"])


@pytest.mark.parametrize("name", IC.CASES)
def test_chunks_of_16_against_one_chunk(name):
    _within_weight_bound(run(name, 40, 16), run(name, 40, 40), f"{name}: chunks of 16 against one of 40")


@pytest.mark.parametrize("name,n,chunk", [("gumbel", 7, 3), ("gumbel-784", 40, 16), ("vae-saturated", 40, 40)])
def test_x_is_not_read_where_it_is_missing(name, n, chunk):
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
    fl, ze = run(name, n, chunk), impute(model, d, flat, (x * (m != 0)).astype(np.uint8), m, n, chunk)
    for k in ("mean", "logw", "draw_index", "draw_z"):
        assert np.array_equal(fl[k], ze[k]), k
    assert np.array_equal(fl["stats"][:, [0, 1, 3]], ze["stats"][:, [0, 1, 3]])
    assert not np.array_equal(fl["stats"][:, 2], ze["stats"][:, 2])


# 7 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,chunk", [("vae", 7, 3), ("gumbel-d99", 40, 16), ("gumbel-784", 40, 16)])
def test_all_ones_mask_is_the_call_without_the_bit(name, n, chunk):
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
    w = impute(model, d, flat, x, np.full_like(m, 255), n, chunk)          # (any non-zero byte counts as observed)
    o = impute(model, d, flat, x, None, n, chunk, bit=False)
    g = _g(w["logw"], o["logw"].astype(np.float64))
    err = np.abs(w["mean"] - o["mean"]).max(axis=1)
    print(f"{name}: g {g.max():.3e} mean difference {err.max():.3e}")
    assert (err <= IC.MEAN_GATE + IR.weight_bound(g)).all()
    assert (w["stats"][:, 2] == 0).all() and (o["stats"][:, 2] == 0).all()
    assert w["tail"][3] == 0 and o["tail"][3] == 0 and w["tail"][2] == 0
    # and it is the posterior-mean reconstruction: the statement without a mask, on the unflipped x
    sx = IR.samples(model, d, p32, x, None, n, M, SEED, STEP)
    ex = IR.estimate(sx["lw"], sx["lam"])
    gx = _g(o["logw"], sx["lw"])
    assert (np.abs(o["mean"] - ex["mean"]).max(axis=1) <= IR.weight_bound(gx) + IC.MEAN_GATE).all()


# 8 --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    import torch
    L = _L()
    model, d, p32, flat, xf, eps, u, m, x = IC.setup("gumbel")
    B, n = x.shape[0], 4
    params, xd = dev(flat, torch.float32), dev(xf, torch.uint8)
    ok = _cdims(d, B, 2)
    ws = torch.zeros(L.impute_workspace_bytes(ok, model, 2) // 4 + 64, dtype=torch.float32, device="cuda")
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    mean, stats, logw, tail, dz = nan(B, d.D), nan(B, 4), nan(B, n), nan(L.TAIL), nan(B, 2, d.L)
    di = torch.full((B, 2), -1, dtype=torch.int64, device="cuda")

    def call(cd, n_draws=2, n_samples=n, tail_=tail, ws_=ws):
        return L.lib.gmvae_impute(C.byref(cd), model, L.ptr(xd), L.ptr(params), n_samples, n_draws, L.ptr(mean), L.ptr(stats),
                                  L.ptr(logw), L.ptr(di), L.ptr(dz), L.ptr(tail_) if tail_ is not None else None,
                                  L.ptr(ws_) if ws_ is not None else None, SEED, STEP, L.current_stream())
    nbytes = C.c_uint64()
    for extra in (L.LIK_GREY_BERNOULLI, L.LIK_CONT_BERNOULLI, L.LIK_GAUSSIAN, L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW):
        for bit in (True, False):
            cd = _cdims(d, B, 2, bit=bit, extra=extra)
            assert call(cd) == -2, (extra, bit)
            assert L.lib.gmvae_impute_workspace_bytes(C.byref(cd), model, 2, C.byref(nbytes)) == -2
    for n_draws in (-1, 17):
        assert call(ok, n_draws=n_draws) == -2
        assert L.lib.gmvae_impute_workspace_bytes(C.byref(ok), model, n_draws, C.byref(nbytes)) == -2
    assert call(ok, n_samples=0) == -2
    assert call(ok, tail_=None) == -1 and call(ok, ws_=None) == -1
    assert call(ok, tail_=tail[1:]) == -4
    torch.cuda.synchronize()
    for t in (mean, stats, logw, tail, dz):
        assert bool(torch.isnan(t).all())
    assert bool((di == -1).all()) and bool((ws == 0).all())
    from gmvae_amd.engine import Engine
    e = Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=1)
    with pytest.raises(ValueError, match="pixel_mask=True"):
        e.impute_posterior(xd, 4, mask=torch.from_numpy(m).cuda())
    with pytest.raises(ValueError, match="n_draws"):
        e.impute_posterior(xd, 4, n_draws=17)


# 9 --------------------------------------------------------------------------------------------------------------
def test_engine_matches_the_abi():
    """Engine.impute_posterior is the C call: the same bits as the ABI run of the case, and imputed = where(mask, x, mean)."""
    import torch
    from gmvae_amd.engine import Engine
    name, n, chunk = "gumbel", 7, 3
    model, d, p32, flat, xf, eps, u, m, x = IC.setup(name)
    e = Engine("gmvae", d.D, d.L, d.K, list(d.hidden), random_seed=SEED, temperature=d.temperature, sigma_min=d.sigma_min,
               pixel_mask=True)
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(flat[:e.P]))
    e.noise_seed, e.global_step = SEED, STEP
    o = e.impute_posterior(torch.from_numpy(xf).cuda(), n, mask=torch.from_numpy(m).cuda(), n_draws=M, chunk=chunk, row0=0,
                           return_logw=True)
    r = run(name, n, chunk)
    assert np.array_equal(o["mean"].cpu().numpy(), r["mean"]) and np.array_equal(o["logw"].cpu().numpy(), r["logw"])
    assert np.array_equal(o["draw_index"].cpu().numpy(), r["draw_index"]) and np.array_equal(o["draw_z"].cpu().numpy(), r["draw_z"])
    assert np.array_equal(torch.stack([o["bound"], o["ess"], o["cond_loglik"], o["max_weight"]], dim=1).cpu().numpy(), r["stats"])
    imp = o["imputed"].cpu().numpy()
    assert np.array_equal(imp[m != 0], xf[m != 0].astype(np.float32)) and np.array_equal(imp[m == 0], r["mean"][m == 0])
    plain = e.impute_posterior(torch.from_numpy(xf).cuda(), n)
    assert plain["draw_index"] is None and plain["logw"] is None and bool((plain["cond_loglik"] == 0).all())


def test_runner_and_model_api(tmp_path, capsys):
    import torch
    from gmvae_amd import run_gmvae
    args = ["--model=gmvae", "--latent_size=8", "--batch_size=32", "--max_steps=11", "--summarise_every=4", f"--logdir={tmp_path}",
            "--random_seed=1", "--synthetic_size=256", "--missing_rate=0.5", "--missing_seed=5"]
    model = run_gmvae.main(["--mode=train"] + args)
    res = run_gmvae.main(["--mode=eval", "--impute_samples=20", "--impute_draws=3"] + args)
    out = capsys.readouterr().out
    keys = ["train/imputation_nll_is", "train/imputation_error_rate_is", "train/imputation_cond_loglik", "train/imputation_ess"]
    for k in keys:
        assert k in out and np.isfinite(res[k]), k
    print({k: res[k] for k in keys + ["train/imputation_nll", "train/imputation_distinct_draws"]})
    assert res["train/imputation_cond_loglik"] <= 0 and 1.0 <= res["train/imputation_ess"] <= 20.0
    assert 0.0 < res["train/imputation_nll"] < 2.0 and 0.0 < res["train/imputation_nll_is"] < 2.0
    assert 0.0 <= res["train/imputation_error_rate_is"] <= 1.0
    # the model API
    x = torch.from_numpy((np.random.default_rng(3).random((6, 784)) < 0.87).astype(np.uint8)).cuda()
    mk = torch.from_numpy(PR.make_mask(6, 784)).cuda()
    imp = model.impute(x, mk, n_samples=20)
    assert imp.shape == x.shape and imp.dtype == torch.float32 and torch.equal(imp[mk != 0], x[mk != 0].to(imp.dtype))
    miss = imp[mk == 0]
    assert bool(((miss > 0) & (miss < 1)).all())
    draws = model.impute(x, mk, n_samples=20, n_draws=3, seed=4)
    assert draws.shape == (6, 3, 784) and draws.dtype == torch.uint8 and bool((draws <= 1).all())
    obs = (mk != 0)[:, None, :].expand_as(draws)
    assert torch.equal(draws[obs], x[:, None, :].expand_as(draws)[obs])
    assert torch.equal(draws, model.impute(x, mk, n_samples=20, n_draws=3, seed=4))
    assert not torch.equal(draws[:, 0], draws[:, 1]) or not torch.equal(draws[:, 1], draws[:, 2])
    sc = model.imputation_scores(x, mk, 20)
    assert sc["n_missing"] == float((mk == 0).sum()) and np.isfinite([sc["nll"], sc["cond_loglik"], sc["ess"]]).all()
    assert 0.0 <= sc["error_rate"] <= 1.0 and sc["cond_loglik"] <= 0
