"""tests/shard_cases.py against itself, without a device: Part A's cases keep every hidden unit away from its ReLU's kink, their
per-step inputs and lambda are what the shard tests need; every Part B entry straddles its boundary, can tell a 32-bit Philox
row from the true one at 10 times the gate the device test applies, sits at the entry point's last admitted row0 where it says
so; and the list of noise sites matches gmvae_amd/csrc."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import shard_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_DIMS = -2


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------- Part A
def test_flag_words_are_the_librarys(L):
    for name in ("OBJ_MARGINAL_Y", "OBJ_MARGINAL_Y_IW", "GRAD_DREG", "OBJ_WEIGHTS", "Y_TEMP_DEV", "Y_STRAIGHT_THROUGH", "OBJ_PIXEL_MASK"):
        assert getattr(SC, name) == getattr(L, name), name
    import hip_util
    assert SC.PRE_TOL == hip_util.PRE_TOL


def test_the_cuts_are_the_issues():
    assert [b - a for a, b in SC.CUTS] == [1, 6, 4] and [SC.ROW0 + a for a, _ in SC.CUTS] == [5, 6, 12]
    assert SC.CUTS[0][0] == 0 and SC.CUTS[-1][1] == SC.B == 11
    assert all(SC.CUTS[i][1] == SC.CUTS[i + 1][0] for i in range(2))


def test_every_family_has_a_case_off_every_multiple_of_4():
    kinds = {f.kind for f in SC.FAMILIES}
    assert kinds == {"mask", "lik", "realx", "count", "weights", "temp", "dreg", "iw"}
    for k in kinds:
        assert any(f.d.D % 4 for f in SC.FAMILIES if f.kind == k), k
    assert {f.mname for f in SC.FAMILIES if f.kind == "mask"} == {"vae", "vae_gmp", "gmvae"}
    assert {f.opt for f in SC.FAMILIES if f.kind == "lik"} == {"grey", "cb", "gauss"}
    assert {f.opt for f in SC.FAMILIES if f.kind == "realx"} == {"fixed", "learned"}
    assert {f.opt for f in SC.FAMILIES if f.kind == "count"} == {"poisson", "nb"}
    assert sum(f.control for f in SC.FAMILIES) == 2 and {f.kind for f in SC.FAMILIES if f.control} == {"mask", "realx"}


@pytest.mark.parametrize("id", list(SC.BY_ID))
def test_no_hidden_unit_sits_on_a_relu_kink(id):
    """No ReLU allowance in the shard-sum comparison: in the fp64 statement of the whole batch (and hence of every shard: a
    pre-activation belongs to one row) every hidden unit has |pre| / sum |a||w| > PRE_TOL."""
    C, _ = SC.statement(id)
    r = SC.min_pre_ratio(C)
    print(f"{id}: min |pre| / sum|a||w| = {r:.3e}")
    assert r > SC.PRE_TOL, (id, r)


@pytest.mark.parametrize("id", [f.id for f in SC.FAMILIES if f.kind == "weights"])
def test_the_floor_is_active_on_both_sides_of_every_cut(id):
    P = SC.problem(id)
    lam = P.extra["weights"][2]
    kl_y = P.extra["kl_y"]
    act = kl_y < lam
    assert np.abs(kl_y - lam).min() > 5e-4
    for _, cut in SC.CUTS[:-1]:
        assert act[:cut].any() and act[cut:].any(), (id, cut, act)
        assert not act[cut:].all() and (cut == 1 or not act[:cut].all()), (id, cut, act)
    assert not act.all()
    C, _ = SC.statement(id)                      # ... and the statement at that lambda floors exactly those examples
    assert np.array_equal(np.asarray(C["floor"]) != 0, act), (C["floor"], act)


def test_per_step_inputs_are_the_shards_own_rows():
    P = SC.problem("mask-gumbel-d99")
    m = P.extra["mask"]
    assert m.shape == (SC.B, 99) and len({m[a:b].tobytes() for a, b in SC.CUTS}) == 3
    for a, b in SC.CUTS:
        assert np.array_equal(P.inputs(a, b)["pixel_mask"], m[a:b])
        assert (99 * a) % 4 or a == 0                 # the shard's mask rows start off every multiple of 4 in the batch
    assert m[0].sum() == 0                            # (the one-row shard observes nothing)
    for id in ("f32-gmvae-d99", "nb-vae-d13-s3"):
        P = SC.problem(id)
        assert P.x.dtype == np.float32 and P.x.shape[1] % 4
    for f in SC.FAMILIES:
        P = SC.problem(f.id)
        per = SC.rows_per_example(f)
        assert P.eps.shape == (SC.B * per, f.d.L) and (P.u is None or P.u.shape == (SC.B * f.d.S, f.d.K))
        e, _ = O.noise(per, f.d.L, f.d.K, (SC.ROW0 + 7) * per, SC.SEED, SC.STEP)
        assert np.array_equal(P.eps[7 * per:8 * per], e)          # shard 3's first example draws the whole batch's rows


@pytest.mark.parametrize("id", [f.id for f in SC.FAMILIES if f.kind == "realx"])
def test_float_cases_are_within_reach_of_fp32(id):
    """realx_ref.terms_in: the same statement evaluated in torch fp32 on the CPU measures what the conditioning of a case costs
    ANY fp32 evaluation.  The shard cases are held to the standing gates without an allowance, so that cost stays below a
    quarter of each gate."""
    import torch
    import realx_ref as RR
    P = SC.problem(id)
    C, _ = SC.statement(id)
    a, b = (RR.terms_in(dt, P.model, P.d, P.p32, P.extra["t"], P.eps, P.u, sigma=P.f.sigma, rho=P.extra["rho"])
            for dt in (torch.float32, torch.float64))
    cost = {"loss": abs(a["loss"] - b["loss"]) / (1e-4 * max(abs(C["loss"]), C["nll_abs"])),
            "nll": abs(a["nll"] - b["nll"]) / (1e-4 * C["nll_abs"]), "kl": abs(a["kl"] - b["kl"]) / (1e-4 * max(abs(C["kl"]), 1.0))}
    print(f"{id}: torch fp32 on the CPU, error / gate: {cost}")
    assert abs(b["kl"] - C["kl"]) <= 1e-9 * max(abs(C["kl"]), 1.0) and max(cost.values()) <= 0.25, (id, cost)


def test_straight_through_argmax_is_stable():
    import ytemp_ref as TR
    C, _ = SC.statement("temp-st-d99-s3")
    assert C["gap"].min() > TR.MIN_GAP


# ------------------------------------------------------------------------------------------------------------- Part B
def _margin_of_the_truncated_reference(e):
    if e.site == "step":
        return SC.margin_step(e, SC.step_reference(e, wrong=True), SC.step_reference(e))
    if e.site == "impute":
        return SC.margin_impute(SC.impute_reference(e, wrong=True)[0]["lw"], SC.impute_reference(e)[0]["lw"])
    if e.site == "aggregate_posterior":
        return SC.margin_aggpost(SC.aggpost_reference(e, wrong=True)[0], SC.aggpost_reference(e)[0])
    if e.site in ("ais", "ais_reverse", "refine", "simulate"):
        return SC.margin_noise(SC.chain_noise(e, wrong=True), SC.chain_noise(e))
    return SC.margin_eval(e, SC.eval_reference(e, wrong=True), SC.eval_reference(e))


@pytest.mark.parametrize("id", list(SC.HIGH_BY_ID))
def test_entry_straddles_its_boundary_and_separates(id):
    e = SC.HIGH_BY_ID[id]
    rows, bnd = SC.rows_of(e), SC.BOUNDARIES[e.boundary]
    if e.boundary == "last":
        assert (e.row0 + e.B) * e.per < SC.TWO38 <= (e.row0 + 1 + e.B) * e.per          # the largest admissible row0
        assert rows[0] >> 32 == 0x3F == rows[-1] >> 32                                # the top of the 6-bit high field
    else:
        assert rows[0] < bnd <= rows[-1]
        b = next(b for b in range(e.B) if (e.row0 + b + 1) * e.per > bnd)
        assert 0 < b < e.B - 1                                                        # rows of the call on both sides
        if e.n:
            assert (e.row0 + b) * e.per < bnd                                         # one example's samples straddle it
        if e.site in ("iw_bound_enum_y", "posterior_y") and e.boundary == "2^32":
            assert (e.row0 + e.B) * e.n < bnd                                         # the product with K does the crossing
    assert SC.truncated(rows, e) != rows
    assert e.B <= 24 and e.n <= 7 and SC.CHAIN_C == 2 and SC.CHAIN_T <= 4
    m = _margin_of_the_truncated_reference(e)
    print(f"{id}: the reference at the truncated rows misses the gate {m:.1f} times over")
    assert m > SC.SEPARATION, (id, m)


@pytest.mark.parametrize("cid", SC.TRAIN_CORNERS)
def test_train_corner_straddles_2_32_and_separates(cid):
    e = SC.train_entry(cid)
    rows = SC.rows_of(e)
    assert rows[0] < SC.TWO32 <= rows[-1] and e.row0 % e.B == 0 and SC.GC.BY_ID[cid].kind == "train"
    m = SC.margin_step(e, SC.step_reference(e, wrong=True), SC.step_reference(e))
    print(f"{cid}: the first step at the truncated rows misses the step's gates {m:.1f} times over")
    assert m > SC.SEPARATION
    mine = SC.GC.BY_ID[cid]
    smaller = [c.id for c in SC.GC.CORNERS if c.kind == "train" and c.sched == mine.sched and c.model == mine.model
               and c.fl_inside == mine.fl_inside and c.B < mine.B and SC.TWO32 % c.B]
    assert not smaller, smaller


@pytest.mark.parametrize("name,out_row0", SC.BINARIZE)
def test_binarize_case_crosses_its_boundary_and_separates(name, out_row0):
    """The contract is bit for bit: a 32-bit (31-bit) quad index changes pixels of the rows past the boundary."""
    qpr = SC.BIN_D // 4
    first, last = out_row0 * qpr, (out_row0 + SC.BIN_B) * qpr - 1
    if name == "last":
        assert last == (1 << 62) - 1                   # (the counter's second word carries the stream bit 0x40000000 above it)
    else:
        assert first < SC.BOUNDARIES[name] <= last - qpr
    _, ref = SC.binarize_case(out_row0)
    _, bad = SC.binarize_case(out_row0, wrong=SC.TWO31 if name == "2^31" else SC.TWO32)
    assert int((ref != bad).sum()) >= 10 and set(np.unique(ref)) <= {0, 1}
    if name != "last":
        below = (SC.BOUNDARIES[name] - first) // qpr
        assert np.array_equal(ref[:below], bad[:below]) and (ref[below:] != bad[below:]).any()


def test_every_site_has_its_three_boundaries():
    seen = {}
    for e in SC.HIGH_ROWS:
        seen.setdefault(e.id.rsplit("-", 1)[0], set()).add(e.boundary)
    assert all(v == set(SC.BOUNDARIES) for v in seen.values()), seen
    words = {SC.GC.BY_ID[c].sched for c in SC.STEP_CORNERS}
    assert words == {c.sched for c in SC.GC.CORNERS if c.kind == "step"}               # one corner per leading schedule word
    assert {SC.GC.BY_ID[c].model for c in SC.STEP_CORNERS if c.startswith("mega-") and c.endswith("D16")} == set(SC.GC.MODELS)


def _step_dims(L, e, row0):
    model, d, flat, p32, x = SC.step_setup(e)
    cd = L.make_dims(e.B, d.D, d.L, d.K, d.hidden, S=d.S, sched_flags=e.flags)
    cd.row0 = row0
    return cd, model


def test_last_admissible_row0_is_the_last(L):
    """The step's size call knows the limit, (row0 + B) S [K with y summed out] < 2^38, under every objective: each step entry's
    row0 is admitted and the next one is GMVAE_E_DIMS.  The evaluators check (row0 + B) n [K] < 2^38 in the call itself: the table's
    arithmetic is held here, and tests/test_shards.py makes the refused call on real buffers."""
    size = C.c_uint64()
    steps = [e for e in SC.HIGH_ROWS if e.site == "step" and e.boundary == "last"]
    assert len(steps) == len(SC.STEP_CORNERS) + len(SC.STEP_DIMS)
    for e in steps:
        for row0, want in ((e.row0, 0), (e.row0 + 1, E_DIMS)):
            cd, model = _step_dims(L, e, row0)
            assert L.lib.gmvae_workspace_bytes(C.byref(cd), model, C.byref(size)) == want, (e.id, row0, want)
    for B, K in ((8, 3), (5, 7)):                       # ... and with y summed out at S = 1: (row0 + B) K < 2^38
        last = (SC.TWO38 - 1) // K - B
        for row0, want in ((last, 0), (last + 1, E_DIMS)):
            cd = L.make_dims(B, 100, 5, K, (24,), sched_flags=SC.OBJ_MARGINAL_Y)
            cd.row0 = row0
            assert L.lib.gmvae_workspace_bytes(C.byref(cd), L.MODEL_GMVAE, C.byref(size)) == want, (B, K, row0, want)
    for e in SC.HIGH_ROWS:
        if e.boundary == "last":
            assert (e.row0 + e.B) * e.per < SC.TWO38 <= (e.row0 + 1 + e.B) * e.per, e.id


# ---- the noise sites
_DEF = re.compile(r"^(?!//|#|\}|\s).*?\b(\w+)\s*\(")


def noise_callers():
    """{(file, function)} of every call of noise_vals in gmvae_amd/csrc: the function is the nearest definition above the call
    that starts in column 0."""
    out = set()
    src = os.path.join(ROOT, "gmvae_amd", "csrc")
    for fn in sorted(os.listdir(src)):
        if not fn.endswith((".hpp", ".hip", ".h")):
            continue
        lines = open(os.path.join(src, fn)).read().split("\n")
        for i, line in enumerate(lines):
            if "noise_vals(" not in line or line.lstrip().startswith("//"):
                continue
            for j in range(i, -1, -1):
                head = re.sub(r"__launch_bounds__\([^)]*\)", "", lines[j])
                m = _DEF.match(head)
                if m:
                    out.add((fn, m.group(1)))
                    break
            else:
                raise AssertionError(f"{fn}:{i + 1}: no enclosing function found")
    out.discard(("aux.hpp", "noise_vals"))                  # its own definition
    return out


def test_the_site_list_names_every_caller_of_noise_vals():
    listed = {(f, fn) for f, fn, _ in SC.NOISE_SITES}
    assert len(listed) == len(SC.NOISE_SITES)
    assert noise_callers() == listed
    held = {e.id.rsplit("-", 1)[0] for e in SC.HIGH_ROWS} | set(SC.TRAIN_CORNERS)
    for f, fn, by in SC.NOISE_SITES:
        assert set(by) <= held, (f, fn, by)
    assert {(f, fn) for f, fn, by in SC.NOISE_SITES if not by} == SC.NOT_HELD
