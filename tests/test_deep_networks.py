"""-m gpu: the general schedule (csrc/gmvae_hip.hip run_step_impl) on deep networks, up to the 8 hidden layers the C ABI takes, and
on a full table of slab ranges -- the cases of tests/deep_cases.py against the fp64 statements, at the project's own gates.

  1  the slab-range sweep: depth 1..8 x two width lists x five model / objective forms, 512 rows each, with GMVAE_NSPLIT_SMALL=3
     (so that the small weight gradients ask for their own slab count and the 16-entry table fills) and again without it; the
     plain forms through hip_util.compare_step, the y-summed-out ones through hip_step(flags=) + tail_gates + check_grads against
     tests/ymarg_ref.py / ymarg_iw_ref.py (what tests/test_ymarg.py and test_ymarg_iw.py do); and two steps at 6800 rows, where
     the many-splits count sets in by itself
  3  middle layers on the row-panel kernels (rows_nn_bf6, rows_ws) at R >= 2048, with the launch names of gmvae_step_profile
  4  four hidden layers under every objective family, through the family's own harness
  5  eight hidden layers end to end: forward, every sub-network, the chunked bounds, a 3-step train graph, the guarded arena

No tolerance is this file's own.  profiles/deep_networks_notes.md has the figures test_deep_networks_report prints."""
import ctypes as C

import numpy as np
import pytest
import torch

import deep_cases as DC
import oracle as O

pytestmark = pytest.mark.gpu

SWITCHES = ("GMVAE_NSPLIT_SMALL", "GMVAE_NO_PLANES", "GMVAE_NO_RWS", "GMVAE_NSPLIT_TOP", "GMVAE_PLANES_MINROWS", "GMVAE_PLANES_EXACT",
            "GMVAE_FORCE_CFG")
REPORT = {}          # (sweep case id, GMVAE_NSPLIT_SMALL) -> (schedule, entries in the table, worst error / gate, worst gradient error / gate)
PANELS = {}          # panel case id -> gmvae_step_profile's names


@pytest.fixture(scope="module")
def H():
    import hip_util
    return hip_util


@pytest.fixture(scope="module")
def L():
    from gmvae_amd import _lib
    return _lib


def _env(monkeypatch, pairs=()):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in pairs:
        monkeypatch.setenv(k, v)


def _params(model, d, seed):
    """tests/test_hip_parity.py test_step_matches_oracle's preparation: Xavier weights, biases drawn at 0.05."""
    rng = np.random.default_rng(seed)
    p = O.init_params(model, d, rng)
    for k in p:
        if k.endswith("/b"):
            p[k] = rng.normal(0, 0.05, p[k].shape)
    return p


# ------------------------------------------------------------------------------------------------- 1. the slab-range sweep
_SWEEP_REF = {}      # case id -> what both runs of a y-summed-out case share: inputs and the fp64 statement's (C, g), left unchanged


def _summed_out_step(H, L, c):
    """One step with y summed out against its statement: hip_step under the objective bit, tail_gates, check_grads.  Returns
    (worst term error / gate, worst gradient error / gate)."""
    import ymarg_iw_ref as YI
    import ymarg_ref as YM
    model, d, B, S, K = O.MODEL_GMVAE, c.d, c.B, c.d.S, c.d.K
    iw = bool(c.flags & L.OBJ_MARGINAL_Y_IW)
    statement = (lambda p, x, eps, m=None: YI.loss_and_grads(d, p, x, eps, S, relu_masks=m)) if iw else \
        (lambda p, x, eps, m=None: YM.loss_and_grads(d, p, x, eps, relu_masks=m))
    if c.id not in _SWEEP_REF:
        flat = O.pack(model, d, _params(model, d, c.nh), np.float32)
        x, _, _ = O.make_inputs(d, B, model, seed_x=100 + c.nh)
        eps = np.random.default_rng(c.nh + 1).standard_normal((B * S * K, d.L)).astype(np.float32)
        p32 = O.unpack(model, d, flat.astype(np.float64))
        _SWEEP_REF[c.id] = (flat, x, eps, p32, statement(p32, x, eps))
    flat, x, eps, p32, (Cc, g) = _SWEEP_REF[c.id]
    gs, tail, masks = H.hip_step(model, d, flat, x, eps, None, 5, 3, want_masks=True, flags=c.flags, mask_rows=S * K)
    H.tail_gates(c.id, tail, B, Cc)
    errs = H.check_grads(c.id, model, d, gs, g, B, masks, Cc["pre"], lambda m: statement(p32, x, eps, m)[1])
    terms = max(abs(tail[0] / B - Cc["loss"]) / abs(Cc["loss"]), abs(tail[1] / B - Cc["nll"]) / abs(Cc["nll"]),
                abs(tail[2] / B - Cc["kl"]) / max(abs(Cc["kl"]), 1.0), abs(tail[3] / B - Cc["nent"]) / max(abs(Cc["nent"]), 1.0)) / 1e-4
    return terms, max(e for _, e in errs) / 1e-4


def _plain_step(H, c):
    model = O.MODEL_NAMES[c.model]
    x, eps, u = O.make_inputs(c.d, c.B, model)
    n = len(H.MARGINS)
    H.compare_step(model, c.d, _params(model, c.d, c.nh), x, eps, u)
    new = H.MARGINS[n:]
    return max(v for k, v in new if not k.startswith("grad")), max(v for k, v in new if k.startswith("grad"))


@pytest.mark.parametrize("c", DC.SWEEP, ids=[c.id for c in DC.SWEEP])
def test_sweep_step_matches_fp64_statement(c, monkeypatch, H, L):
    """The step of every sweep case on the general schedule, with the small weight gradients forced to 3 slabs (NSS != NS: the
    table of slab ranges fills as deep_cases.expected_ranges says) and with that switch unset (only the products over the batch
    rows ask), each inside the gates.  A site that writes another number of slabs than finalize_grads adds for its range is a
    wrong gradient tensor here."""
    model = O.MODEL_NAMES[c.model]
    for forced in (DC.NSPLIT_SMALL, None):
        _env(monkeypatch, DC.ENV if forced else DC.ENV[1:])
        cd = H.dims_of(c.d, c.B)
        cd.sched_flags = c.flags
        sched = L.step_schedule(cd, model)
        assert sched.startswith("general"), sched
        try:
            terms, grads = _summed_out_step(H, L, c) if c.flags else _plain_step(H, c)
        except AssertionError:
            REPORT[c.id, forced] = (sched, c.ranges(forced).fill, float("nan"), float("nan"))
            raise
        REPORT[c.id, forced] = (sched, c.ranges(forced).fill, terms, grads)


@pytest.mark.parametrize("mname,d,B", DC.THRESHOLD_CASES, ids=[f"{m}-S{d.S}-B{B}" for m, d, B in DC.THRESHOLD_CASES])
def test_many_splits_at_their_default_threshold_with_a_ragged_first_layer(mname, d, B, monkeypatch, H, L):
    """No switch set: at R = 6800 rows the small weight gradients take 17 slabs by themselves, the rest 16 (or num_splits(B) = 6),
    and D * hidden[0] % 4 != 0 puts the last x row and the first y row of encoder_gmm's first layer into one float4."""
    _env(monkeypatch)
    model = O.MODEL_NAMES[mname]
    assert L.step_schedule(H.dims_of(d, B), model) == "general"
    x, eps, u = O.make_inputs(d, B, model)
    H.compare_step(model, d, _params(model, d, B), x, eps, u)


# ------------------------------------------------------------------------------ 3. middle layers on the row-panel paths
def _profile_names(H, L, model, d, flat, x, eps, u):
    """The launch names of one step, from gmvae_step_profile (one timed iteration)."""
    B = x.shape[0]
    cd = H.dims_of(d, B)
    P, _ = L.param_count(cd, model)
    params, xd = H.dev(flat, torch.float32), H.dev(x, torch.uint8)
    ed, ud = H.dev(eps, torch.float32), (None if u is None else H.dev(u, torch.float32))
    grads = torch.zeros(P + L.TAIL, dtype=torch.float32, device="cuda")
    ws = H.workspace(cd, model)
    n, names = C.c_int(), C.create_string_buffer(96 * 48)
    usec, flops = (C.c_float * 96)(), (C.c_double * 96)()
    L.check(L.lib.gmvae_step_profile(C.byref(cd), model, L.ptr(xd), L.ptr(ed), L.ptr(ud), L.ptr(params), L.ptr(grads), L.ptr(ws), 0, 1,
                                     96, C.byref(n), names, usec, flops, L.current_stream()), "gmvae_step_profile")
    torch.cuda.synchronize()
    return tuple(names.raw[i * 48:(i + 1) * 48].split(b"\0")[0].decode() for i in range(n.value))


@pytest.mark.parametrize("c", DC.PANEL_CASES, ids=[c.id for c in DC.PANEL_CASES])
def test_middle_layers_on_the_row_panel_kernels(c, monkeypatch, H, L):
    """Three and four hidden layers at R >= 2048 rows, every switch at its default: the per-row hidden layers run in rows_nn_bf6
    and rows_ws (deep_cases.per_row_forward_kernels; tests/test_deep_networks_cpu.py), a middle layer on each, the decoder's
    data gradients ping-pong through dbuf over three and four layers.  Against the oracle, and the launches by name."""
    _env(monkeypatch)
    model = O.MODEL_NAMES[c.model]
    assert L.step_schedule(H.dims_of(c.d, c.B), model) == "general"
    p = _params(model, c.d, c.B)
    x, eps, u = O.make_inputs(c.d, c.B, model)
    H.compare_step(model, c.d, p, x, eps, u)
    names = _profile_names(H, L, model, c.d, O.pack(model, c.d, p, np.float32), x, eps, u if model == O.MODEL_GMVAE else None)
    PANELS[c.id] = names
    assert names == c.names


# ------------------------------------------------------------------------------- 4. depth under every objective family
def _family_dims(**kw):
    return O.Dims(**{**DC.FAMILY_DIMS, **kw})


def test_four_layers_marginal_y(L):
    import test_ymarg as T
    d = _family_dims()
    flat, x, eps = T._setup(d, DC.FAMILY_B, seed=4)
    assert L.step_schedule(T._mdims(d, DC.FAMILY_B), O.MODEL_GMVAE) == "general+marginal"
    T.compare_step(d, flat, x, eps, "deep marginal")


def test_four_layers_marginal_y_iw(L):
    import test_ymarg_iw as T
    d = _family_dims()
    flat, x, eps = T._setup(d, DC.FAMILY_B, 2, seed=4)
    assert L.step_schedule(T._idims(d, DC.FAMILY_B, 2), O.MODEL_GMVAE) == "general+marginal_iw"
    T.compare_step(d, 2, flat, x, eps, "deep marginal_iw")


def test_four_layers_labels_with_dreg(L):
    import test_semisup as T
    d, B, S = _family_dims(), DC.FAMILY_B, 2
    flags = L.OBJ_MARGINAL_Y_IW | L.OBJ_LABELS | L.GRAD_DREG
    flat, x, eps = T._setup(d, B, S, seed=6)
    y = T._labels(d.K, B, 6)
    assert L.step_schedule(T._sdims(d, B, S, flags=flags), O.MODEL_GMVAE) == "general+marginal_iw+labels+dreg"
    _, _, Cc = T.compare_step(d, S, flat, x, eps, y, T.ALPHA, "deep labels+dreg", flags=flags, estimator="dreg")
    assert 2 <= Cc["n_labelled"] < B


def test_four_layers_vae_dreg():
    import test_dreg as T
    model, d, B, S = O.MODEL_VAE, _family_dims(K=1), DC.FAMILY_B, 3
    flat, x, eps = T._setup(model, d, B, S, seed=8)
    T.check_step("deep vae dreg", dict(model=model, d=d, B=B, S=S, flat=flat, x=x, eps=eps,
                                       dreg=T.dstep(model, d, S, flat, x, eps, T._L().GRAD_DREG)))


def test_four_layers_weights_temperature_straight_through(monkeypatch, L):
    """GMVAE_OBJ_WEIGHTS | GMVAE_Y_TEMP_DEV | GMVAE_Y_STRAIGHT_THROUGH: tests/test_ytemp.py's comparison on a case of this depth
    (its table is keyed by name: the case is added for the call and taken out again)."""
    import test_ytemp as T
    import ytemp_ref as TR
    name = "deep-weights"
    monkeypatch.setitem(TR.CASES, name, (_family_dims(), DC.FAMILY_B, 42))
    try:
        ws, cd, Cc = T.compare_step(name, 0.5, True)
    finally:
        for k in [k for k in T._REF if k[0] == name]:
            del T._REF[k]
    assert cd.sched_flags == L.OBJ_WEIGHTS | L.Y_TEMP_DEV | L.Y_STRAIGHT_THROUGH
    assert L.step_schedule(cd, O.MODEL_GMVAE) == "general+weights+temp+st"


def test_four_layers_pixel_mask(monkeypatch):
    """tests/test_pmask.py's step test (the gates, the held-out terms, the exact zeros of the dead columns) on a case of this depth."""
    import pmask_ref as PR
    import test_pmask as T
    name = "deep"
    monkeypatch.setitem(PR.CASES, name, PR.Case("gmvae", _family_dims(), DC.FAMILY_B))
    try:
        T.test_step_matches_fp64_statement(name)
    finally:
        T._REF.pop(name, None)


def test_four_layers_real_valued_with_learned_scale(monkeypatch):
    """GMVAE_LIK_GAUSSIAN | GMVAE_X_F32 | GMVAE_LIK_SCALE_LEARNED: tests/test_realx.py's step test on a case of this depth."""
    import realx_ref as RR
    import test_realx as T
    name = "deep"
    monkeypatch.setitem(RR.CASES, name, RR.Case("gmvae", _family_dims(), DC.FAMILY_B))
    try:
        T.test_step_matches_fp64_statement(name, "learned")
    finally:
        T._REF.pop((name, "learned"), None)


def test_four_layers_clip_norm(monkeypatch):
    """GMVAE_OPT_CLIP_NORM: tests/test_clip.py's eager train step (the record and the clipped TF-Adam update against
    tests/clip_ref.py and adam_ref.py, clipping and not) on an engine of this depth."""
    import test_clip as T
    f = DC.FAMILY_DIMS
    case = dict(model="gmvae", D=f["D"], Lz=f["L"], K=f["K"], hidden=f["hidden"], B=DC.FAMILY_B, kw={})
    monkeypatch.setitem(T.CASES, "deep", case)
    monkeypatch.setitem(T.ALL, "deep", case)
    T.test_eager_train_step_is_the_statement("deep")


@pytest.mark.parametrize("mname,act", [("gmvae", "tanh"), ("vae_gmp", "elu")])
def test_four_layers_other_activations(mname, act, H, L):
    model, d = O.MODEL_NAMES[mname], _family_dims(act=act)
    assert L.step_schedule(H.dims_of(d, DC.FAMILY_B), model) == "general"
    x, eps, u = O.make_inputs(d, DC.FAMILY_B, model)
    H.compare_step(model, d, _params(model, d, 3), x, eps, u)


# ------------------------------------------------------------------------------------- 5. eight hidden layers end to end
MODELS = ("gmvae", "vae", "vae_gmp")
NETS = {"gmvae": ("ENCODER_Y", "PRIOR_GMM", "ENCODER_GMM", "DECODER"), "vae": ("ENCODER", "DECODER"), "vae_gmp": ("ENCODER", "DECODER")}


def _eight(mname, **kw):
    return O.Dims(**{**DC.EIGHT, "K": 1 if mname == "vae" else DC.EIGHT["K"], **kw})


@pytest.mark.parametrize("mname", MODELS)
def test_eight_layers_forward(mname, H):
    """gmvae_forward's rows, samples and tail against oracle.forward, at tests/test_hip_parity.py test_forward_outputs' tolerances."""
    model, d, B = O.MODEL_NAMES[mname], _eight(mname, S=2), DC.EIGHT_B
    flat = O.pack(model, d, _params(model, d, 5), np.float32)
    x, eps, u = O.make_inputs(d, B, model)
    Cc = O.forward(model, d, O.unpack(model, d, flat.astype(np.float64)), x, eps, u)
    tail, rows, z, y, lg = H.hip_forward(model, d, flat, x, eps, u)
    np.testing.assert_allclose(z, Cc["z"], rtol=1e-4, atol=1e-5)
    if model == O.MODEL_GMVAE:
        np.testing.assert_allclose(y, Cc["y"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(lg, Cc["logits"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(rows[:, 0], Cc["logpx"], rtol=1e-5)
    np.testing.assert_allclose(rows[:, 3], Cc["logw"], rtol=1e-5)
    assert tail[0] / B == pytest.approx(Cc["loss"], rel=1e-5)


@pytest.mark.parametrize("mname,net", [(m, n) for m in MODELS for n in NETS[m]], ids=lambda v: str(v).lower())
def test_eight_layers_mlp_forward(mname, net, H, L):
    """gmvae_mlp_forward of every sub-network on 9 rows against snt.nets.MLP restated in fp64 (oracle._mlp_fwd), at
    tests/test_memory_contract.py test_mlp_forward_stays_inside_its_buffers' tolerances."""
    from oracle import gmvae_oracle as OO
    rows, model, d = 9, O.MODEL_NAMES[mname], _eight(mname, gen_bias_init=-0.3)
    rng = np.random.default_rng(rows + len(net))
    flat = O.pack(model, d, _params(model, d, rows + len(net)), np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    x = (rng.random((rows, d.D)) < 0.6).astype(np.uint8)
    y = rng.dirichlet(np.ones(d.K), rows).astype(np.float32)
    z = rng.standard_normal((rows, d.L)).astype(np.float32)
    nl = len(d.hidden) + 1
    inp, in2, out_dim, ref = {
        "ENCODER_Y": lambda: (x, None, d.K, OO._mlp_fwd(p32, "encoder_y", nl, x.astype(np.float64))[0]),
        "PRIOR_GMM": lambda: (y, None, 2 * d.L, OO._mlp_fwd(p32, "prior_gmm", 1, y.astype(np.float64))[0]),
        "ENCODER_GMM": lambda: (x, y, 2 * d.L, OO._mlp_fwd(p32, "encoder_gmm", nl, np.concatenate([x, y], 1).astype(np.float64))[0]),
        "DECODER": lambda: (z, None, d.D, OO._mlp_fwd(p32, "decoder", nl, z.astype(np.float64))[0] + d.gen_bias_init),
        "ENCODER": lambda: (x, None, 2 * d.L, OO._mlp_fwd(p32, "encoder", nl, x.astype(np.float64))[0]),
    }[net]()
    u8 = inp.dtype == np.uint8
    cd = H.dims_of(d, rows)
    params, ind = H.dev(flat, torch.float32), H.dev(inp, torch.uint8 if u8 else torch.float32)
    in2d = None if in2 is None else H.dev(in2, torch.float32)
    od = torch.full((rows, out_dim), float("nan"), dtype=torch.float32, device="cuda")
    ws = H.workspace(cd, model)
    L.check(L.lib.gmvae_mlp_forward(C.byref(cd), model, getattr(L, f"NET_{net}"), L.ptr(ind), int(u8), L.ptr(in2d), rows, L.ptr(params),
                                    L.ptr(od), L.ptr(ws), L.current_stream()), "gmvae_mlp_forward")
    torch.cuda.synchronize()
    np.testing.assert_allclose(od.cpu().numpy(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("mname", MODELS)
def test_eight_layers_iw_bound(mname):
    """gmvae_iw_bound at n = 5 samples in chunks of 2 (a ragged last chunk) against tests/test_iw_bound.py's oracle statement."""
    import test_iw_bound as T
    model, d, B = O.MODEL_NAMES[mname], _eight(mname), 5
    flat = O.pack(model, d, _params(model, d, 6), np.float32)
    x, _, _ = O.make_inputs(d, B, model, seed_x=106)
    ref = T.oracle_bound(f"deep-{mname}", model, d, flat, x, 5)
    bound, mlw, tail = T.iw(model, d, flat, x, 5, 2)
    assert np.all(np.abs(bound - ref) <= 1e-4 * np.abs(ref)), (bound, ref)
    assert np.all(mlw <= bound + 1e-4 * np.abs(bound))
    assert tail[4] == B and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * abs(tail[0])


def test_eight_layers_iw_bound_enum_y():
    """gmvae_iw_bound_enum_y at n = 5 in chunks of 2 against tests/test_iw_enum.py's fp64 statement."""
    import test_iw_enum as T
    d, B = _eight("gmvae"), 5
    flat, x = T._setup(d, B)
    ref, ref_mlw = T.fp64_bound("deep", d, flat, x, 5)
    bound, mlw, tail = T.enum(d, flat, x, 5, 2)
    assert np.all(np.abs(bound - ref) <= 1e-4 * np.abs(ref)), (bound, ref)
    assert np.all(np.abs(mlw - ref_mlw) <= 1e-4 * np.abs(ref_mlw)), (mlw, ref_mlw)
    assert np.all(mlw <= bound)
    assert tail[4] == B and abs(-tail[0] - bound.astype(np.float64).sum()) <= 1e-5 * abs(tail[0]) and np.all(tail[5:] == 0)


@pytest.mark.parametrize("mname", MODELS)
def test_eight_layers_train_graph(mname):
    """Three steps of a train graph (finalize_grads_adam behind eight layers of slab ranges) against three oracle steps."""
    import test_timed_path as T
    d = _eight(mname)
    T.trajectory_case(mname, d.D, d.L, d.K, d.hidden, DC.EIGHT_B, 3)


@pytest.mark.parametrize("mname", MODELS)
def test_eight_layers_step_inside_the_guarded_arena(mname, H, L):
    """The step with every buffer in a guarded arena, the workspace at exactly gmvae_workspace_bytes: the gates and the guards."""
    import arena as A
    model, d, B = O.MODEL_NAMES[mname], _eight(mname), DC.EIGHT_B
    ar = A.Arena("cuda", 1 << 24)
    x, eps, u = O.make_inputs(d, B, model)
    H.compare_step(model, d, _params(model, d, 7), x, eps, u, alloc=ar)          # (run_checked: GuardHit on any byte outside)
    cd = H.dims_of(d, B)
    assert ar.buf("workspace").nbytes == L.workspace_bytes(cd, model)
    assert ar.buf("grads").nbytes == 4 * (L.param_count(cd, model)[0] + L.TAIL)


def test_deep_networks_report():
    """Not a gate: what the cases above measured in this process (file order, run with -s) -- per sweep case the schedule, the
    entries expected in the table of slab ranges, the worst term and the worst gradient error over their gates; per row-panel case
    the launch names.  The source of the tables in profiles/deep_networks_notes.md."""
    print()
    for (cid, forced), (sched, fill, terms, grads) in REPORT.items():
        print(f"[deep] {cid:28s} NSPLIT_SMALL {forced or '-':>2} {sched:20s} table {fill:2d}  terms / gate {terms:.3f}  grads / gate {grads:.3f}")
    for cid, names in PANELS.items():
        print(f"[deep panel] {cid}: {' '.join(names)}")
