"""No GPU: tests/deep_cases.py against itself and against the library's sizing entry points, and the two fp64 statements against
each other at the depth the C ABI allows (GMVAE_MAX_HIDDEN = 8).

  the bookkeeping   expected_ranges (the 16-entry SlabX table of the general schedule's backward pass, restated site by site)
                    against the table of first refusals read off run_step_impl, and the sweep of tests/test_deep_networks.py
                    against the edges it exists for: per site one case where the request just fits and one where the site is the
                    first to be turned away, and the two cases whose entry is dropped without asking
  the row panels    the three middle-layer cases reach rows_nn_bf6 and rows_ws on a middle layer, by the gates as restated
  the ABI's edge    oracle.loss_and_grads against objective_ref (torch autograd) at 4 and 8 hidden layers, the layout at 8 layers,
                    9 layers refused by every sizing entry point, the kept activations' offsets up to layer 8"""
import ctypes as C

import numpy as np
import pytest

import deep_cases as DC
import objective_ref as OR
import oracle as O


def _lib():
    from gmvae_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------ the bookkeeping
def test_constants_are_the_librarys():
    L = _lib()
    assert (DC.OBJ_MARGINAL_Y, DC.OBJ_MARGINAL_Y_IW, DC.MAX_HIDDEN) == (L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.MAX_HIDDEN)


@pytest.mark.parametrize("c", DC.SWEEP, ids=[c.id for c in DC.SWEEP])
def test_sweep_case_is_what_the_sweep_assumes(c, monkeypatch):
    """512 rows (two slabs by default, one for the products over the batch rows), the general schedule under the sweep's
    switches, no weight beyond small_ns' 131072 outputs, and a table that never holds more than 16 entries."""
    L = _lib()
    for k, v in DC.ENV:
        monkeypatch.setenv(k, v)
    assert c.rows == 512 and DC.num_splits(c.rows) == 2 and DC.num_splits(c.B) == 1
    cd = L.make_dims(c.B, c.d.D, c.d.L, c.d.K, c.d.hidden, S=c.d.S, sched_flags=c.flags)
    assert L.step_schedule(cd, O.MODEL_NAMES[c.model]).startswith("general")
    assert L.workspace_bytes(cd, O.MODEL_NAMES[c.model]) > 0
    dims = (c.d.D + c.d.K, c.d.L) + tuple(c.d.hidden) + (2 * c.d.L, c.d.D)
    assert max(dims) ** 2 <= DC.SMALL_OUTS
    r = c.ranges()
    assert (r.NS, r.NSS) == (2, 3) and r.NSB == (1 if c.d.S > 1 else 2)
    assert r.fill <= DC.SLAB_RANGES and all(s.before <= DC.SLAB_RANGES for s in r.sites)
    # without GMVAE_NSPLIT_SMALL the small sites want the default count: only the products over the batch rows ask
    r0 = c.ranges(None)
    assert r0.NSS == r0.NS and all(s.site in ("layer0_x", "layer0_y", "encoder") for s in r0.sites if s.want)
    assert (c.d.D * c.d.hidden[0]) % 4 == (0 if c.widths == "A" else 2)


@pytest.mark.parametrize("form", list(DC.FIRST_REFUSED))
@pytest.mark.parametrize("w", list(DC.WIDTHS))
def test_first_refusal_by_depth(form, w):
    """expected_ranges against the table read off the code: which site is the first to find the table full, per depth."""
    for nh, want in DC.FIRST_REFUSED[form].items():
        s = DC.SWEEP_BY_ID[f"{form}-{w}-nh{nh}"].ranges().first_refused
        assert (s.site if s else None) == want, (form, w, nh, s)


def test_entry_counts_of_the_plain_forms():
    """The counts the table of first refusals rests on: 2 per decoder layer, 2 per upper layer of encoder_gmm, 2 + 1 for layer 0,
    2 for the prior, 2 per encoder layer -- 15 entries for a one-hidden-layer GMVAE, 16 exactly for a three-layer VAE and for a
    three-layer GMVAE behind the x rows of layer 0."""
    assert DC.SWEEP_BY_ID["gmvae-gumbel-A-nh1"].ranges().fill == 15
    assert DC.SWEEP_BY_ID["vae-A-nh3"].ranges().fill == 16 and DC.SWEEP_BY_ID["vae-A-nh3"].ranges().first_refused is None
    r = DC.SWEEP_BY_ID["gmvae-gumbel-A-nh3"].ranges()
    x = next(s for s in r.sites if s.site == "layer0_x")
    assert x.granted and x.before + x.want == 16 and r.first_refused.site == "layer0_y" and r.first_refused.before == 16
    # a refused site writes and reads the default count; a granted one its own
    for c in DC.SWEEP:
        for s in c.ranges().sites:
            if s.want and s.granted:
                assert s.written == s.read != 2
            elif c.id not in DC.DROPPED_ENTRIES or s.site != "layer0_y":
                assert s.written == s.read == 2, (c.id, s)


@pytest.mark.parametrize("site", DC.SITES)
def test_sweep_reaches_both_edges_of_every_site(site):
    """Per site: a case where its request just fits (the table at 14, 15 or 16 behind it) and a case where it is the first to be
    turned away.  (Layer 0: its x rows ask with 4 nh + 2 entries in the table -- 6, 10, 14, or 18 with an upper layer already
    turned away -- so they fit or are not the first; the first refusal of the site is its y rows', at nh = 3.)"""
    fits = [c.id for c in DC.SWEEP if c.ranges().just_fits(site)]
    first = [c.id for c in DC.SWEEP if (c.ranges().first_refused and c.ranges().first_refused.group == site)]
    assert fits and first, (site, fits, first)
    if site == "layer0":
        rs = [c.ranges() for c in DC.SWEEP]
        assert any(s.site == "layer0_x" and s.granted and s.before + s.want == 16 for r in rs for s in r.sites)
        assert any(s.site == "layer0_y" and s.granted and s.before + s.want == 15 for r in rs for s in r.sites)
        assert all(r.first_refused.site == "layer0_y" for r in rs if r.first_refused and r.first_refused.group == "layer0")


def test_sweep_holds_the_entries_that_are_dropped_without_asking():
    """nh = 3, widths B, S > 1: the y rows take the x rows' one slab, the table is full behind the x rows' two entries, and the y
    rows' entry is dropped -- their launch writes 1 slab, finalize_grads adds 2 (the second a slab nothing writes: zero in the
    workspace the contract asks for).  With the Gumbel draw and with y summed out over S = 2 samples, and in no other case."""
    for cid in DC.DROPPED_ENTRIES:
        c = DC.SWEEP_BY_ID[cid]
        assert (c.widths, c.nh) == ("B", 3) and c.d.S > 1 and (c.d.D * c.d.hidden[0]) % 4 != 0
        (s,) = c.ranges().dropped
        assert (s.site, s.before, s.want, s.granted, s.written, s.read) == ("layer0_y", 16, 1, False, 1, 2)
        assert not c.ranges(None).dropped
    assert "gmvae-marginal_iw-B-nh3" in DC.DROPPED_ENTRIES                       # (y summed out: ymarg_dw)
    assert tuple(k.id for k in DC.SWEEP if k.ranges().dropped) == DC.DROPPED_ENTRIES
    assert not any(k.ranges(None).dropped for k in DC.SWEEP)
    # the same shapes with widths A ask like every other site (and are turned away); one layer less and the entry fits
    for cid in DC.DROPPED_ENTRIES:
        assert not DC.SWEEP_BY_ID[cid.replace("-B-", "-A-")].ranges().dropped
        y = next(s for s in DC.SWEEP_BY_ID[cid.replace("nh3", "nh2")].ranges().sites if s.site == "layer0_y")
        assert y.granted and (y.written, y.read) == (1, 1)
    # S = 1 (y summed out, one sample): the x rows keep the default count and so do the y rows, whatever small_ns would grant
    y = next(s for s in DC.SWEEP_BY_ID["gmvae-marginal-B-nh1"].ranges().sites if s.site == "layer0_y")
    assert (y.want, y.written, y.read) == (0, 2, 2)


def test_threshold_cases_take_many_splits_with_no_switch_set(monkeypatch):
    """6800 rows: the small weight gradients take 17 slabs against the default 16 by themselves, and the x rows of layer 0 either
    keep the default (S = 1) or take num_splits(B) = 6 (S = 4); the y rows follow the x rows across the float4 they share."""
    L = _lib()
    monkeypatch.delenv("GMVAE_NSPLIT_SMALL", raising=False)
    assert DC.num_splits_small(6799) == 16 and DC.num_splits_small(6800) == 17
    for (mname, d, B), nsx in zip(DC.THRESHOLD_CASES, (16, 6)):
        assert B * d.S == 6800 and (d.D * d.hidden[0]) % 4 != 0
        assert L.step_schedule(L.make_dims(B, d.D, d.L, d.K, d.hidden, S=d.S), O.MODEL_NAMES[mname]) == "general"
        r = DC.expected_ranges(mname, d, B)
        assert (r.NS, r.NSS, r.NSB) == (16, 17, nsx) and not r.dropped
        assert (r.first_refused.site if r.first_refused else None) == (None if d.S == 1 else "encoder")      # (15 entries, as in the sweep at nh = 2)
        by = {s.site: s for s in r.sites}
        assert by["layer0_x"].written == by["layer0_y"].written == nsx and by["prior"].written == by["decoder"].written == 17


# ------------------------------------------------------------------------------------------------------ the row panels
def test_panel_cases_put_a_middle_layer_on_each_row_panel_kernel(monkeypatch):
    L = _lib()
    monkeypatch.delenv("GMVAE_NO_PLANES", raising=False)
    seen = set()
    for c in DC.PANEL_CASES:
        nh = len(c.d.hidden)
        assert nh >= 3 and c.B >= 2048 and (c.B % 128 == 0) == c.plane_rows
        cd = L.make_dims(c.B, c.d.D, c.d.L, c.d.K, c.d.hidden)
        # (the plane launches' own size gates -- a top layer of 256 inputs at least, D >= 512 -- keep them off at D = 256)
        assert L.step_schedule(cd, O.MODEL_NAMES[c.model]) == "general"
        ks = DC.per_row_forward_kernels(c.model, c.d, c.B)
        middle = {k: v for k, v in ks.items() if 0 < k[1] < (nh - 1 if k[0] == "decoder" else nh)}
        assert middle and "gemm_grouped" not in ks.values()
        seen |= set(middle.values())
        if c.model == "gmvae":
            assert ks["decoder", 1] == "rows_ws" and ks["encoder_gmm", 2] == "rows_nn_bf6" and c.names.count("bwd_enc_gmm_dh") == 1
    assert seen == {"rows_nn_bf6", "rows_ws"}
    # one row fewer than 2048 and every such layer is the grouped GEMM's
    c = DC.PANEL_CASES[0]
    assert set(DC.per_row_forward_kernels(c.model, c.d, 2047).values()) == {"gemm_grouped"}


# ------------------------------------------------------------------------------------------------------ the ABI's edge
TERM_RTOL = 1e-12      # tests/test_objective_ref_cpu.py RTOL: of max(|value|, 1) for a scalar, of the tensor's largest magnitude


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "elu"])
@pytest.mark.parametrize("mname", ["gmvae", "vae", "vae_gmp"])
@pytest.mark.parametrize("nh", [4, 8])
def test_the_two_fp64_statements_agree_on_deep_networks(nh, mname, act):
    """oracle.loss_and_grads (numpy, the hand-derived backward) against objective_ref (torch autograd): the loss, its terms and
    every gradient tensor, at S = 2."""
    model = O.MODEL_NAMES[mname]
    d = O.Dims(D=48, L=6, K=1 if mname == "vae" else 5, hidden=DC.WIDTHS["A"][0][:nh], S=2, act=act, temperature=0.8)
    rng = np.random.default_rng(nh)
    p = O.init_params(model, d, rng)
    for k in p:
        if k.endswith("/b"):
            p[k] = rng.normal(0, 0.05, p[k].shape)
    x, eps, u = O.make_inputs(d, 7, model)
    Co, go = O.loss_and_grads(model, d, p, x, eps, u, np.float64)
    kw = dict(u=u) if model == O.MODEL_GMVAE else {}
    c, g = OR.loss_and_grads(model, d, p, x, eps, OR.iwae, S=d.S, **kw)
    terms = {"loss": c["loss"], "nll": -c["logpx"].mean().item(), "kl": (c["logq"] - c["logp"]).mean().item(),
             "nent": c["nent"].mean().item()}
    for k, v in terms.items():
        assert abs(v - Co[k]) <= TERM_RTOL * max(abs(Co[k]), 1.0), (k, v, Co[k])
    assert set(g) == set(go)
    for k in go:
        assert np.abs(go[k]).max() > 0, k
        assert np.abs(g[k] - go[k]).max() <= TERM_RTOL * np.abs(go[k]).max(), k


@pytest.mark.parametrize("mname", ["gmvae", "vae", "vae_gmp"])
def test_layout_at_eight_hidden_layers_is_the_oracles(mname):
    L = _lib()
    model = O.MODEL_NAMES[mname]
    d = O.Dims(**{**DC.EIGHT, "K": 1 if mname == "vae" else DC.EIGHT["K"]})
    cd = L.make_dims(DC.EIGHT_B, d.D, d.L, d.K, d.hidden)
    assert cd.n_hidden == DC.MAX_HIDDEN
    lay, P, _ = O.param_layout(model, d)
    got = L.param_layout(cd, model)
    assert len(lay) == len(got)
    for (n, s, o), (n2, s2, o2) in zip(lay, got):          # (the oracle's vectors are [n], the library's [1, n])
        assert (n, o, int(np.prod(s))) == (n2, o2, s2[0] * s2[1]) and tuple(s)[-1] == s2[1]
    assert L.param_count(cd, model)[0] == P
    nets = 3 if mname == "gmvae" else 2
    assert sum(n.endswith("/w") for n, _, _ in got) == nets * 9 + (1 if mname == "gmvae" else 0)


def _nine(L, flags=0):
    """Dims of nine hidden layers: the struct holds eight widths, n_hidden says nine."""
    cd = L.make_dims(DC.EIGHT_B, DC.EIGHT["D"], DC.EIGHT["L"], DC.EIGHT["K"], DC.EIGHT["hidden"], sched_flags=flags)
    cd.n_hidden = DC.MAX_HIDDEN + 1
    return cd


def test_nine_hidden_layers_are_refused():
    L = _lib()
    with pytest.raises(ValueError):
        L.make_dims(4, 48, 6, 5, (16,) * 9)
    u64, n = C.c_uint64(), C.c_int()
    E_DIMS = -2
    assert L.ERRORS[E_DIMS] == "GMVAE_E_DIMS"
    for model in (L.MODEL_GMVAE, L.MODEL_VAE, L.MODEL_VAE_GMP):
        for flags in (0, L.OBJ_MARGINAL_Y) if model == L.MODEL_GMVAE else (0,):
            r = C.byref(_nine(L, flags))
            assert L.lib.gmvae_param_count(r, model, C.byref(u64), C.byref(C.c_uint64())) == E_DIMS
            assert L.lib.gmvae_param_layout(r, model, None, 0, C.byref(n)) == E_DIMS
            assert L.lib.gmvae_workspace_bytes(r, model, C.byref(u64)) == E_DIMS
            assert L.lib.gmvae_iw_bound_workspace_bytes(r, model, C.byref(u64)) == E_DIMS
            assert L.lib.gmvae_workspace_offset(r, model, b"slabs", C.byref(u64)) == E_DIMS
            assert L.lib.gmvae_step_schedule(r, model, C.create_string_buffer(48)) == E_DIMS
    r = C.byref(_nine(L))
    assert L.lib.gmvae_iw_bound_enum_y_workspace_bytes(r, L.MODEL_GMVAE, C.byref(u64)) == E_DIMS
    assert L.lib.gmvae_posterior_y_workspace_bytes(r, L.MODEL_GMVAE, C.byref(u64)) == E_DIMS
    assert L.lib.gmvae_posterior_component_workspace_bytes(r, L.MODEL_VAE_GMP, C.byref(u64)) == E_DIMS
    # eight are sized by every one of them
    cd = L.make_dims(DC.EIGHT_B, DC.EIGHT["D"], DC.EIGHT["L"], DC.EIGHT["K"], DC.EIGHT["hidden"])
    for q in (L.workspace_bytes, L.iw_bound_workspace_bytes, L.iw_bound_enum_y_workspace_bytes, L.posterior_y_workspace_bytes):
        assert q(cd, L.MODEL_GMVAE) > 0
    assert L.posterior_component_workspace_bytes(cd, L.MODEL_VAE_GMP) > 0


def test_kept_activations_have_offsets_up_to_layer_eight():
    """gmvae_workspace_offset "he<i>" / "hg<i>" / "hd<i>": the kept input activation of layer i, i = 1 .. 8 at eight hidden
    layers -- distinct, inside the workspace, each behind the one before by at least its own bytes; layer 9 is refused."""
    L = _lib()
    d, B = O.Dims(**DC.EIGHT), DC.EIGHT_B
    cd = L.make_dims(B, d.D, d.L, d.K, d.hidden)
    total = L.workspace_bytes(cd, L.MODEL_GMVAE)
    for tag in ("he", "hg", "hd"):
        offs = [L.workspace_offset(cd, L.MODEL_GMVAE, f"{tag}{i}") for i in range(1, 9)]
        assert len(set(offs)) == 8 and all(o % 16 == 0 for o in offs)
        for i, o in enumerate(offs):
            assert o + 4 * B * d.hidden[i] <= total
        spans = sorted((o, o + 4 * B * d.hidden[i]) for i, o in enumerate(offs))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        with pytest.raises(L.GmvaeError):
            L.workspace_offset(cd, L.MODEL_GMVAE, f"{tag}9")
    # with fewer layers the layers behind the last are refused too
    cd4 = L.make_dims(B, d.D, d.L, d.K, d.hidden[:4])
    assert L.workspace_offset(cd4, L.MODEL_GMVAE, "hd4") > 0
    with pytest.raises(L.GmvaeError):
        L.workspace_offset(cd4, L.MODEL_GMVAE, "hd5")
