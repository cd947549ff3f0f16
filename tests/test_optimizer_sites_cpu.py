"""No device: the fp64 TF-Adam statement and its bounds (tests/adam_ref.py) on their own, before tests/test_optimizer_sites.py
holds every fused optimizer site of the library to them.

  * the fp32 NumPy statement (oracle.adam_tf_step) stays inside the bounds over every hyperparameter set, step counter and state;
  * the fp32 form of alpha_t (-expm1f, csrc/dwadam.hpp and csrc/skinny.hpp) is measured against the fp64 form on the same matrix;
  * three wrong statements -- eps behind the bias correction (torch's placement), t off by one, b1 and b2 swapped -- leave the
    bounds on at least a tenth of the matrix's elements under every hyperparameter set: the bounds can tell them apart."""
import numpy as np
import pytest

import adam_ref as A
import oracle as O

P = 4000
STEPS = [t0 + 1 for t0 in A.T0] + [A.T0_WRAP + 1, A.T0_WRAP + 2, A.T0_WRAP + 3]      # every t a device test applies
FIRST_STEPS = [t0 + 1 for t0 in A.T0 + (A.T0_WRAP,)]                                   # one per step counter t0 of the matrix


def _case(t, seed):
    """(p, m, v, gsum, count) of one cell of the matrix: the warm state of its counter, gradients spanning 1e-9 .. 1e2."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.1, 0.1, size=P).astype(np.float32)
    m, v = A.warm_state(P, t - 1, seed + 1)
    count = (1, 17, 24, 1024)[seed % 4]
    g = (rng.choice([-1.0, 1.0], size=P) * 10.0 ** rng.uniform(-9, 2, size=P) * count).astype(np.float32)
    g[::37] = 0
    return p, m, v, g, count


def _outside(got, case, t, hp, d_alpha=A.D_ALPHA_FP64):
    """Elements where (p', m', v') = got leaves the bounds of the right statement."""
    p, m, v, g, count = case
    p2, m2, v2, _ = A.predict(p, m, v, g, count, t, *hp)
    dm, dv, dp = A.bounds(p, m, v, g, count, t, *hp, d_alpha=d_alpha)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got[0] - p2) <= dp) & (np.abs(got[1] - m2) <= dm) & (np.abs(got[2] - v2) <= dv)
    return ~ok


@pytest.mark.parametrize("hp_id", sorted(A.HP))
def test_fp32_numpy_statement_stays_inside_the_bounds(hp_id):
    lr, b1, b2, eps = A.HP[hp_id]
    for k, t in enumerate(STEPS):
        case = _case(t, 10 * hp_id + k)
        p, m, v, g, count = case
        gj = g * (np.float32(1) / np.float32(count))                   # as the device forms it
        got = O.adam_tf_step(p, m, v, gj, t, lr=float(np.float32(lr)), b1=b1, b2=b2, eps=eps, dtype=np.float32)
        bad = _outside(got, case, t, A.HP[hp_id])
        assert not bad.any(), (hp_id, t, int(bad.sum()), int(np.argmax(bad)))


@pytest.mark.parametrize("hp_id", sorted(A.HP))
def test_fp32_numpy_statement_with_gradients_below_the_underflow_threshold(hp_id):
    """Gradients of 1e-30 .. 1e-19 on the zero state and on the warm one: gj^2 is a subnormal fp32 number or 0, so v' of the
    fp32 statement is off by up to a subnormal spacing whatever its size.  The bounds hold with their TINY terms -- and the
    relative count alone (4u (gj^2 + v)) does not on the zero state: that is what the terms are for."""
    lr, b1, b2, eps = A.HP[hp_id]
    for t in (1, 1000):
        rng = np.random.default_rng(100 * hp_id + t)
        p = rng.uniform(-0.1, 0.1, size=P).astype(np.float32)
        m, v = A.warm_state(P, t - 1, hp_id)
        count = (1, 24)[t == 1000]
        g = (rng.choice([-1.0, 1.0], size=P) * 10.0 ** rng.uniform(-30, -19, size=P) * count).astype(np.float32)
        case = (p, m, v, g, count)
        gj = g * (np.float32(1) / np.float32(count))
        got = O.adam_tf_step(p, m, v, gj, t, lr=float(np.float32(lr)), b1=b1, b2=b2, eps=eps, dtype=np.float32)
        bad = _outside(got, case, t, A.HP[hp_id])
        assert not bad.any(), (hp_id, t, int(bad.sum()), int(np.argmax(bad)))
        if t == 1:
            _, _, v2, _ = A.predict(p, m, v, g, count, t, *A.HP[hp_id])
            dv = A.bounds(p, m, v, g, count, t, *A.HP[hp_id])[1] - 4 * A.TINY
            assert (np.abs(got[2] - v2) > dv).any(), "the relative count alone holds here: the TINY terms would be unused"


def test_fp32_alpha_form_against_the_fp64_form():
    """d_alpha over every (t, b1, b2) of the matrix: finite and below 1e-5 (profiles/optimizer_sites_notes.md has the table)."""
    rows = []
    for hp_id, (lr, b1, b2, eps) in sorted(A.HP.items()):
        for t in STEPS:
            d = A.d_alpha_fp32(t, b1, b2)
            rows.append((hp_id, t, d))
            print(f"d_alpha hp{hp_id} b1={b1} b2={b2} t={t}: {d:.3e}")
    bad = [r for r in rows if not (np.isfinite(r[2]) and r[2] < 1e-5)]
    assert not bad, bad


def _torch_eps(p, m, v, gj, t, lr, b1, b2, eps):
    m2 = m + (gj - m) * A.one_minus(b1)
    v2 = v + (gj * gj - v) * A.one_minus(b2)
    b1, b2 = np.float64(np.float32(b1)), np.float64(np.float32(b2))
    mh, vh = m2 / (1 - b1 ** t), v2 / (1 - b2 ** t)
    return p - np.float64(np.float32(lr)) * mh / (np.sqrt(vh) + np.float64(np.float32(eps))), m2, v2


WRONG = {
    "eps-after-bias-correction": lambda p, m, v, g, c, t, hp: _torch_eps(p, m, v, g / c, t, *hp),
    "t-off-by-one": lambda p, m, v, g, c, t, hp: A.predict(p, m, v, g, c, t + 1, *hp)[:3],
    "betas-swapped": lambda p, m, v, g, c, t, hp: A.predict(p, m, v, g, c, t, hp[0], hp[2], hp[1], hp[3])[:3],
}


@pytest.mark.parametrize("wrong", sorted(WRONG))
@pytest.mark.parametrize("hp_id", sorted(A.HP))
def test_bounds_reject_a_wrong_statement(hp_id, wrong):
    """Evaluated EXACTLY (fp64), each wrong statement leaves the bounds on >= 10 % of the elements of the matrix's states under
    this hyperparameter set, pooled over the matrix's five step counters, one state each (behind t ~ 1e5 the bias corrections
    are 1 to fp64 precision: neither the eps placement nor t + 1 changes the update there at all, under any set).  The bounds use the widest allowance a site gets:
    the fp32 form's d_alpha."""
    hp = A.HP[hp_id]
    out = n = 0
    for k, t in enumerate(FIRST_STEPS):
        case = _case(t, 10 * hp_id + k)
        p, m, v, g, count = (np.asarray(a, np.float64) for a in case)
        got = WRONG[wrong](p, m, v, g, count, t, hp)
        out += int(_outside(got, case, t, hp, d_alpha=max(A.D_ALPHA_FP64, A.d_alpha_fp32(t, hp[1], hp[2]))).sum())
        n += P
    print(f"hp{hp_id} {wrong}: outside the bounds on {out / n:.1%} of {n} elements")
    assert out >= 0.10 * n, (hp_id, wrong, out / n)
