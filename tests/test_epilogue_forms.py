"""The top decoder layer's loss epilogues in every tile configuration on the device (tests/epilogue_cases.py has the table and the
derivation of its shapes): seven families -- the masked Bernoulli, the three likelihoods on bytes, the Gaussian on float x and /
or under the learned scale -- x GMVAE_FORCE_CFG = 0, 1, 2 (32 x 32 with K split over 4 waves, 64 x 64, 128 x 128 as the big-round
instance and as the general loop) x the interior, quad-predicated, ragged-row and unaligned paths of a tile, each step against
the family's fp64 statement at the family's standing gates, unchanged:

    mask    hip_util.tail_gates, tail[5] at 1e-4 of itself, tail[6..7] exact, the dead columns exactly 0 (tests/test_pmask.py)
    lik     test_lik.lik_gates and sq_gates
    realx   the same two, rho's gradient at 1e-4 of its max, its pad 0 (tests/test_realx.py)
    all     every gradient tensor at 1e-4 of its own max (hip_util.check_grads, with the device-mask recompute)

Evidence that a forced configuration ran: per case the gradient buffers under the three configurations are pairwise NOT
bit-identical and agree to 2e-4 of max |g| (test_hip_parity.test_big_round_gemm_inside_the_step_iwae's bound); on "whole" the
general 128 x 128 loop (GMVAE_NO_BIG=1) differs in bits from the big-round instance.  gmvae_forward -- no C output: the
`Cout == nullptr` instantiations -- runs test_forward_row_terms' comparison on "ragged" under 64 x 64 and 128 x 128.

Measured on an MI355X: profiles/epilogue_forms_notes.md."""
import ctypes as C
import itertools

import numpy as np
import pytest

import epilogue_cases as EC
import gate_corners as G
import realx_ref as RR
from hip_util import _L, check_grads, dev, device_masks, dims_of, tail_gates, workspace, write_inputs
from test_lik import lik_gates, sq_gates
from test_pmask import _dead_zeros

pytestmark = pytest.mark.gpu

MARGINS = {}       # (family, configuration) -> {gate: worst error / gate over the shapes}: test_epilogue_forms_report prints it
# The cases whose per-row terms from gmvae_forward miss the standing gate for their conditioning alone, under test_realx.CONDITIONED's
# rule: realx_ref.real_batch's x 30 columns drive encoder_gmm's raw scale far below 0, where sigma_q = softplus(.) is a denormal
# fp32 number and ln sigma_q keeps a few bits in ANY fp32 evaluation.  The allowance is measured, not chosen: 4x the error of the
# same statement in torch fp32 on the CPU (realx_ref.terms_in) or the standing gate, whichever is larger.  Measured, the same
# under 64 x 64 and 128 x 128 (profiles/epilogue_forms_notes.md): gauss-f32-lsig-ragged log q: device 0.930, torch fp32 4.75 (188x
# the standing gate of the worst row); log p(x|z), log p and log w sit inside the standing gates (0.002, 0.012 and 0.007 of them).
# No other term and no STEP case takes an allowance: every one sits inside the standing gates.
CONDITIONED = {("gauss-f32-lsig", "ragged"): ("logq",)}      # (case: the terms that take the allowance)


def _force(monkeypatch, cfg, no_big=False):
    for k in G.SWITCHES + ("GMVAE_FORCE_CFG", "GMVAE_NO_BIG", "GMVAE_NO_PLANES", "GMVAE_PLANES_MINROWS", "GMVAE_NSPLIT_SMALL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GMVAE_FORCE_CFG", str(cfg))
    if no_big:
        monkeypatch.setenv("GMVAE_NO_BIG", "1")


def _call(I, entry):
    """One gmvae_step (explicit noise, seed 5, step 3) or gmvae_forward on the case's inputs under the current environment.
    step: (grad sums [P] float64, tail [8], the step's ReLU masks, the gradient buffer's fp32 bits); forward: (rows [R, 4], tail)."""
    import torch
    L = _L()
    cd = dims_of(I.d, I.B)
    cd.sched_flags = I.flags
    assert L.step_schedule(cd, I.model).startswith("general+")
    P, _ = L.param_count(cd, I.model)
    assert P == I.flat.shape[0]
    params, xd, ed = dev(I.flat, torch.float32), dev(I.x), dev(I.eps, torch.float32)
    assert xd.dtype == (torch.float32 if EC.FAMILIES[I.family].f32 else torch.uint8)
    ud = None if I.u is None else dev(I.u, torch.float32)
    ws = workspace(cd, I.model)
    if I.regions:
        write_inputs(ws, cd, I.model, I.regions)
    if entry == "step":
        grads = torch.full((P + L.TAIL,), float("nan"), dtype=torch.float32, device="cuda")
        L.check(L.lib.gmvae_step(C.byref(cd), I.model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws), 5, 3,
                                 None, L.current_stream()), "gmvae_step")
        torch.cuda.synchronize()
        raw = grads.cpu().numpy()
        g = raw.astype(np.float64)
        return g[:P], g[P:], device_masks(ws, cd, I.model, I.d, I.B), raw[:P]
    R = I.B * I.d.S
    tail = torch.full((L.TAIL,), float("nan"), device="cuda")
    rows = torch.full((R, 4), float("nan"), device="cuda")
    L.check(L.lib.gmvae_forward(C.byref(cd), I.model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(tail), L.ptr(rows), None,
                                None, None, L.ptr(ws), 0, 0, L.current_stream()), "gmvae_forward")
    torch.cuda.synchronize()
    return rows.cpu().numpy().astype(np.float64), tail.cpu().numpy().astype(np.float64)


def _tail_margins(I, Cc, tail):
    """Each tail gate's error over the gate itself (figures for the notes; the standing functions below do the asserting)."""
    B = I.B
    if EC.FAMILIES[I.family].kind == "mask":
        return {"loss": abs(tail[0] / B - Cc["loss"]) / (1e-4 * abs(Cc["loss"])), "nll": abs(tail[1] / B - Cc["nll"]) / (1e-4 * abs(Cc["nll"])),
                "kl": abs(tail[2] / B - Cc["kl"]) / (1e-4 * max(abs(Cc["kl"]), 1.0)),
                "nent": abs(tail[3] / B - Cc["nent"]) / (1e-4 * max(abs(Cc["nent"]), 1.0)),
                "tail5": abs(tail[5] - Cc["hid"]) / (1e-4 * abs(Cc["hid"]))}
    mag = Cc["nll_abs"]
    return {"loss": abs(tail[0] / B - Cc["loss"]) / (1e-4 * max(abs(Cc["loss"]), mag)), "nll": abs(tail[1] / B - Cc["nll"]) / (1e-4 * mag),
            "kl": abs(tail[2] / B - Cc["kl"]) / (1e-4 * max(abs(Cc["kl"]), 1.0)),
            "nent": abs(tail[3] / B - Cc["nent"]) / (1e-4 * max(abs(Cc["nent"]), 1.0)),
            "tail5": abs(tail[5] - Cc["sqerr"]) / (1e-4 * abs(Cc["sqerr"]))}


def _record(I, cfg, m):
    what = f"{I.family}-{I.shape}-cfg{cfg}"
    print(f"{what}: error / gate " + " ".join(f"{k} {v:.3f}" for k, v in m.items()))
    worst = MARGINS.setdefault((I.family, str(cfg)), {})
    for k, v in m.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _tail_gates(I, what, Cc, tail):
    B, D = I.B, I.d.D
    assert np.isfinite(tail).all()
    if EC.FAMILIES[I.family].kind == "mask":
        tail_gates(what, tail, B, Cc)
        assert abs(tail[5] - Cc["hid"]) <= 1e-4 * abs(Cc["hid"]), (what, tail[5], Cc["hid"])
        assert tail[6] == Cc["n_missing"] and tail[7] == Cc["n_observed"]
    else:
        lik_gates(what, tail, B, Cc)
        sq_gates(what, tail, B, D, Cc)


def _step_gates(I, Cc, g, cfg, gs, tail, masks):
    fam = EC.FAMILIES[I.family]
    what = f"{I.family}-{I.shape}-cfg{cfg}"
    assert np.isfinite(gs).all()
    m = _tail_margins(I, Cc, tail)
    _tail_gates(I, what, Cc, tail)
    P0 = I.flat.shape[0] - (RR.pad4(I.d.D) if fam.learned else 0)
    errs = check_grads(what, I.model, I.d, gs[:P0], g, I.B, masks, Cc["pre"], lambda mk: EC.statement(I, mk)[1])
    m["grads"] = max(e for _, e in errs) / 1e-4
    if fam.kind == "mask":
        _dead_zeros(I.model, I.d, gs, what)
    if fam.learned:
        D = I.d.D
        got, ref = gs[P0:P0 + D] / I.B, g[RR.LOG_SIGMA]
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
        print(f"{what} {RR.LOG_SIGMA}: rel-to-max err {err:.3e}")
        m["rho"] = err / 1e-4
        assert err <= 1e-4, (what, err)
        assert not gs[P0 + D:].any()                                # (the pad behind rho's D values)
    _record(I, cfg, m)


# 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", EC.STEP_CASES, ids=[f"{f}-{s}" for f, s in EC.STEP_CASES])
def test_step_in_every_tile_configuration(family, shape, monkeypatch):
    I, (Cc, g) = EC.case(family, shape)
    bits = {}
    runs = [(str(c), c, False) for c in EC.CFGS] + ([("2-general", 2, True)] if shape == "whole" else [])
    for tag, cfg, no_big in runs:
        _force(monkeypatch, cfg, no_big)
        gs, tail, masks, raw = _call(I, "step")
        _step_gates(I, Cc, g, tag, gs, tail, masks)
        bits[tag] = raw
    # the forced configurations ran: no two of them left the same bits, and all of them the same gradient
    for a, b in itertools.combinations(bits, 2):
        assert not np.array_equal(bits[a], bits[b]), (family, shape, a, b)
        np.testing.assert_allclose(bits[a], bits[b], rtol=0, atol=2e-4 * np.abs(bits[b]).max(), err_msg=f"{family}-{shape} cfg {a} vs {b}")


# 2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape", EC.FORWARD_CASES, ids=[f"{f}-{s}" for f, s in EC.FORWARD_CASES])
def test_forward_row_terms_without_a_c_output(family, shape, monkeypatch):
    """gmvae_forward's per-row log p(x|z), log q, log p and log w and its tail against the statement, under 64 x 64 and
    128 x 128 tiles (the entry point reads GMVAE_FORCE_CFG as gmvae_step does); the two leave different bits."""
    import torch
    I, (Cc, _) = EC.case(family, shape)
    fam = EC.FAMILIES[family]
    ref = Cc["rows"]
    mag = 1.0 if fam.kind == "mask" else max(Cc["nll_abs"], 1.0)      # (logpx and log w: relative to the magnitude of their addends)
    t32 = None
    if fam.kind == "realx":
        t32 = RR.terms_in(torch.float32, I.model, I.d, I.p32, I.t, I.eps, I.u, sigma=EC.SIGMA, rho=I.rho)["rows"]
    seen = {}
    for cfg in EC.FORWARD_CFGS:
        _force(monkeypatch, cfg)
        rows, tail = _call(I, "forward")
        what = f"{family}-{shape}-forward-cfg{cfg}"
        m = _tail_margins(I, Cc, tail)
        _tail_gates(I, what, Cc, tail)
        for j, term in enumerate(("logpx", "logq", "logp", "logw")):
            gate = 1e-4 * np.maximum(np.abs(ref[:, j]), mag if j in (0, 3) else 1.0)
            err = np.abs(rows[:, j] - ref[:, j])
            m[term] = (err / gate).max()
            if t32 is not None:
                e32 = np.abs(t32[:, j] - ref[:, j]).max()
                print(f"{what} {term}: device err max {err.max():.3e}; torch fp32 on the CPU err max {e32:.3e}")
                if term in CONDITIONED.get((family, shape), ()):
                    gate = np.maximum(gate, 4.0 * e32)
            assert (err <= gate).all(), (what, term, err.max())
        if fam.kind == "mask":
            assert (rows[:I.d.S, 0] == 0).all()            # (row 0 observes nothing: its masked logpx is an empty sum)
        _record(I, f"{cfg}-forward", m)
        seen[cfg] = rows
    a, b = (seen[c] for c in EC.FORWARD_CFGS)
    assert not np.array_equal(a[:, 0], b[:, 0]), (family, shape)


def test_epilogue_forms_report():
    """Not a gate: the worst error over its gate per family and configuration, as measured in this process (file order, run
    with -s) -- the source of the table in profiles/epilogue_forms_notes.md."""
    print()
    for (family, cfg), m in sorted(MARGINS.items()):
        print(f"[epilogue forms] {family:15s} cfg {cfg:10s} " + " ".join(f"{k} {v:.3f}" for k, v in m.items()))
