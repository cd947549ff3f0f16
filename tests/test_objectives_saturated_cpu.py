"""The conditions of tests/test_objectives_saturated.py's cases, without a device: asserted on the fp64 statements alone
(tests/saturated_cases.py), with the values printed.  A case that misses one gets another seed or logit scale there, with the
reason in a comment; the conditions stay."""
import numpy as np
import pytest

import saturated_cases as SC
import wobj_ref as WR

FP32_ZERO = 1e-38             # below the smallest normal float32 (1.18e-38): q_bk is zero or denormal on the device
CE_FP32_INF = 104.0           # -ln q_bc above -ln(2^-149) = 103.3: q_bc is exactly 0 in fp32, the cross-entropy is finite
ONE_SAMPLE = 1.0 - 1e-6       # a sample group whose softmax_s weight has collapsed onto one sample


def _path(c):
    """The kernels a case is about: DReG cases count under `dreg` as well as under their objective."""
    return {c.path} | ({"dreg"} if c.dreg else set())


@pytest.mark.parametrize("name", list(SC.CASES))
def test_statement_is_finite_and_both_terms_are_visible(name):
    c, f = SC.CASES[name], SC.facts(name)
    print(f"{name}: {f}")
    assert f["finite"], name
    if c.regime == "trained":          # nll and kl within a factor 100: both sides of the inference gradient inside the gate's view
        assert f["nll"] > 0 and f["kl"] > 0 and 0.01 <= f["nll"] / f["kl"] <= 100.0, (name, f["nll"], f["kl"])
    else:                              # diverging: the KL term is the loss
        assert f["kl"] > 100.0 * f["nll"] or c.mname == "vae", (name, f["nll"], f["kl"])


@pytest.mark.parametrize("path", ["marginal", "marginal_iw", "labels", "weights", "dreg"])
def test_every_path_has_a_case_whose_q_is_zero_in_fp32(path):
    got = {n: SC.facts(n)["min_q"] for n, c in SC.CASES.items() if path in _path(c) and c.mname == "gmvae"}
    print(path, got)
    assert got and min(got.values()) < FP32_ZERO, (path, got)


def test_a_labelled_example_has_a_cross_entropy_beyond_fp32s_smallest_q():
    got = {n: SC.facts(n)["ce_max"] for n in SC.names("labels")}
    print(got)
    assert max(v for v in got.values() if v is not None) > CE_FP32_INF, got
    for regime in SC.REGIMES:          # ... in each regime
        assert max(got[n] for n in SC.names("labels", regime=regime)) > CE_FP32_INF, (regime, got)


def test_a_sample_group_has_collapsed_onto_one_sample():
    got = {n: SC.facts(n)["max_v"] for n, c in SC.CASES.items() if c.S > 1}
    print({n: f"1 - {1 - v:.3e}" for n, v in got.items()})
    assert max(got.values()) > ONE_SAMPLE, got
    for kind in ("marginal_iw", "labels", "dreg"):
        assert max(got[n] for n, c in SC.CASES.items() if c.S > 1 and kind in _path(c)) > ONE_SAMPLE, (kind, got)


@pytest.mark.parametrize("name", [n for n in SC.names("weights") if SC.CASES[n].mname == "gmvae"])
def test_the_floor_holds_where_the_case_says(name):
    c = SC.CASES[name]
    w = SC.weights_of(name)                                    # (split: wobj_ref.split_lambda asserts the gap > 1e-3 nat)
    C, _ = SC.statement(name)
    kl_y, n = C["kl_y"], int(C["floor"].sum())
    print(f"{name}: lambda {w[2]:.6f} KL_y {np.sort(kl_y)} on the floor {n} of {c.B}")
    if c.lam == "split":
        assert WR.split_lambda(kl_y) == w[2] and 0 < n < c.B and np.abs(kl_y - w[2]).min() > 5e-4
    elif c.lam == "all_floor":
        assert n == c.B and (kl_y < w[2] - 1e-3).all()
    else:
        assert w[2] == 0.0 and n == 0


@pytest.mark.parametrize("name", SC.names("labels"))
def test_hits_are_unambiguous_at_fp32(name):
    from test_semisup import TOP2_GAP
    C, _ = SC.statement(name)
    y = SC.labels_of(name)
    gap = C["top2_gap"][C["labelled"]]
    print(f"{name}: labels {y.tolist()} labelled {C['n_labelled']} hits {C['hits']} smallest top-2 gap {gap.min():.3e}")
    assert C["n_labelled"] >= 2 and gap.min() > TOP2_GAP
    c = SC.CASES[name]
    if c.labels == "pattern":
        assert (y == 0).any() and (y == c.d.K - 1).any() and (y == c.d.K).any() and (y == -1).any()
    elif c.labels == "argmax":
        assert C["hits"] == C["n_labelled"] == c.B
    else:
        assert C["hits"] == 0 and C["n_labelled"] == c.B


def test_every_kernel_has_a_case_in_each_regime():
    for regime in SC.REGIMES:
        for kind in ("marginal", "marginal_iw", "labels", "weights", "dreg"):
            assert [n for n, c in SC.CASES.items() if kind in _path(c) and c.regime == regime], (kind, regime)
        w = [SC.CASES[n] for n in SC.names("weights", regime=regime)]
        assert any(c.gumbel for c in w) and any(c.mname == "gmvae" and not c.gumbel for c in w) and any(c.mname != "gmvae" for c in w)


def test_the_forward_only_cases():
    """The posterior's case over y has entries of q(y|x) that are 0 in fp32; both statements are finite."""
    import post_comp_ref as R
    from test_posterior_component import SEED, STEP
    q = SC.q_of("forward-h24x2-trained")
    print("forward-h24x2-trained: min q", q.min(1))
    assert (q < FP32_ZERO).any() and np.isfinite(q).all()
    c, i = SC.FORWARD["forward-vae_gmp-trained"], SC.inputs("forward-vae_gmp-trained")
    lw = R.log_w(c.d, i["flat"], i["x"], SC.FORWARD_N, 0, SEED, STEP)
    print("forward-vae_gmp-trained: log w in", lw.min(), lw.max())
    assert np.isfinite(lw).all()
