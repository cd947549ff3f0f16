"""Deep networks on the general schedule (csrc/gmvae_hip.hip run_step_impl) -- test infrastructure, a plain module: the case tables
of tests/test_deep_networks.py (on the device, against the fp64 statements) and tests/test_deep_networks_cpu.py (the tables
against themselves and against the library's sizing entry points, no device).

The C ABI takes up to GMVAE_MAX_HIDDEN = 8 hidden layers per network and run_step_impl builds its launches in loops over them.
What depth changes in the backward pass is the bookkeeping of the split-K slabs: every weight gradient is written to `ns` slabs
and finalize_grads* (kernels.hpp) adds NS = num_splits(R) of them unless the parameter's range stands in SlabX, a table of
kSlabRanges = 16 entries.  expected_ranges() restates, site by site and in the order run_step_impl visits them, who asks for
entries and who still gets them:

  site               asks for                      when                                       entries
  decoder            NSS slabs (small_ns)          NSS != NS and in * out <= 131072           2 (weight, bias) per layer, top layer first
  encoder_gmm_upper  NSS slabs (small_ns)          the same, layers nh .. 1                   2 per layer
  layer0_x           NSB slabs (nsx)               S > 1 and NSB != NS                        2
  layer0_y           NSS slabs (small_ns)          as the decoder (K * hidden[0] outputs)     1 (no bias) -- but it asks for room for 2
  prior              NSS slabs (small_ns)          as the decoder (K * 2 L outputs)           2
  encoder            NSB slabs (nse)               S > 1 and NSB != NS, layers nh .. 0        2 per layer

A site that does not find `entries asked + table <= 16` writes and registers NS slabs instead: the fallback rule.  One site does
not ask: with (D * hidden[0]) % 4 != 0 the y rows take the x rows' count (finalize_grads adds whole float4s, and the one the two
share is summed over the x rows' slabs) and their entry goes to the table if ONE slot is free; if none is, the entry is dropped
while the launch still writes that count (Ranges.dropped; profiles/deep_networks_notes.md has the verdict).  GMVAE_NO_PLANES=1 is assumed (the
plane top layer would ask for its own count first), and no weight of the sweep has more than 131072 outputs."""
import dataclasses

import oracle as O

MAX_HIDDEN = 8                  # include/gmvae_hip.h GMVAE_MAX_HIDDEN
SLAB_RANGES = 16                # kernels.hpp kSlabRanges
NS_MAX, NS_SMALL_MAX = 16, 64   # gmvae_hip.hip
SMALL_OUTS = 131072             # small_ns: weights of at most this many elements take NSS slabs
OBJ_MARGINAL_Y, OBJ_MARGINAL_Y_IW = 4, 8       # include/gmvae_hip.h (tests/test_deep_networks_cpu.py holds them to gmvae_amd._lib)
ENV = (("GMVAE_NSPLIT_SMALL", "3"), ("GMVAE_NO_PLANES", "1"))      # the sweep's switches; each case runs again without the first
NSPLIT_SMALL = 3

SITES = ("decoder", "encoder_gmm_upper", "layer0", "prior", "encoder")       # (layer0: its x rows and its y rows)


def num_splits(R):
    return max(1, min(NS_MAX, R // 256))


def num_splits_small(R, forced=None):
    """forced: GMVAE_NSPLIT_SMALL (honoured in 1 .. 64)."""
    ns = max(1, min(NS_SMALL_MAX, R // 400))
    return forced if forced is not None and 1 <= forced <= NS_SMALL_MAX else ns


@dataclasses.dataclass(frozen=True)
class Site:
    site: str           # decoder | encoder_gmm_upper | layer0_x | layer0_y | prior | encoder
    layer: int
    want: int           # entries the site would add (0: it wants the default count and asks for nothing)
    before: int         # entries in the table when it asks
    granted: bool       # the entries went into the table
    written: int        # slabs its launch writes
    read: int           # slabs finalize_grads adds for its range

    @property
    def group(self):
        return "layer0" if self.site.startswith("layer0") else self.site


@dataclasses.dataclass(frozen=True)
class Ranges:
    NS: int
    NSB: int
    NSS: int
    sites: tuple

    @property
    def fill(self):
        return sum(s.want for s in self.sites if s.granted)

    @property
    def first_refused(self):
        """The first site that asked and was turned away (None: everything fits)."""
        return next((s for s in self.sites if s.want and not s.granted), None)

    @property
    def dropped(self):
        """Sites whose launch writes another count than finalize_grads reads."""
        return tuple(s for s in self.sites if s.written != s.read)

    def just_fits(self, group):
        """A request of the group that was granted and left the table at 14, 15 or 16 entries."""
        return any(s.group == group and s.want and s.granted and s.before + s.want >= SLAB_RANGES - 2 for s in self.sites)


def expected_ranges(model, d, B, flags=0, nsplit_small=None):
    """The SlabX bookkeeping of one general-schedule step of `model` ("gmvae" | "vae" | "vae_gmp") at dims d (oracle.Dims, d.S
    samples), batch B, objective bits `flags`, GMVAE_NSPLIT_SMALL = nsplit_small (None: unset), planes off."""
    gm = model == "gmvae"
    marg = gm and bool(flags & (OBJ_MARGINAL_Y | OBJ_MARGINAL_Y_IW))
    S, K, Lz, D, nh = d.S, d.K, d.L, d.D, len(d.hidden)
    R = B * S * (K if marg else 1)
    NS = num_splits(R)
    NSB = min(num_splits(B), NS) if S > 1 else NS
    NSS = max(num_splits_small(R, nsplit_small), NS)
    sites, n = [], 0

    def add(site, layer, ns, want, room):
        """ns: the count the site would like; room: the free entries it asks for before it takes `want`."""
        nonlocal n
        if ns == NS:
            sites.append(Site(site, layer, 0, n, False, NS, NS))
            return NS
        ok = n + room <= SLAB_RANGES
        sites.append(Site(site, layer, want, n, ok, ns if ok else NS, ns if ok else NS))
        n += want if ok else 0
        return ns if ok else NS

    def small(outs):
        return NSS if outs <= SMALL_OUTS else NS

    dec = (Lz,) + tuple(d.hidden) + (D,)
    for i in range(nh, -1, -1):
        add("decoder", i, small(dec[i] * dec[i + 1]), 2, 2)
    if gm:
        g = (D + K,) + tuple(d.hidden) + (2 * Lz,)
        for i in range(nh, 0, -1):
            add("encoder_gmm_upper", i, small(g[i] * g[i + 1]), 2, 2)
        nsx = add("layer0_x", 0, NSB if S > 1 else NS, 2, 2)
        if (D * g[1]) % 4:
            # nsy = nsx, whatever small_ns answered; brange takes the entry while one slot is free and drops it otherwise --
            # the y rows' launch (ymarg_dw with y summed out, else the layer-0 GEMM group) writes nsx slabs either way
            if nsx == NS:
                sites.append(Site("layer0_y", 0, 0, n, False, NS, NS))
            else:
                ok = n + 1 <= SLAB_RANGES
                sites.append(Site("layer0_y", 0, 1, n, ok, nsx, nsx if ok else NS))
                n += 1 if ok else 0
        else:
            add("layer0_y", 0, small(K * g[1]), 1, 2)
        add("prior", 0, small(K * 2 * Lz), 2, 2)
    for i in range(nh, -1, -1):
        add("encoder", i, NSB if S > 1 else NS, 2, 2)
    return Ranges(NS, NSB, NSS, tuple(sites))


# ------------------------------------------------------------------------------------------------- 1. the slab-range sweep
WIDTHS = {"A": ((20, 12, 28, 16, 24, 12, 20, 16), 48), "B": ((22, 12, 27, 16, 24, 13, 20, 18), 49)}      # name: (widths, D)
LATENT = 6
FORMS = {       # name: (model, objective bits, B, S, K): R = 512 rows each, num_splits(R) = 2, num_splits(B) = 1
    "gmvae-gumbel": ("gmvae", 0, 128, 4, 5),
    "gmvae-marginal": ("gmvae", OBJ_MARGINAL_Y, 64, 1, 8),
    "gmvae-marginal_iw": ("gmvae", OBJ_MARGINAL_Y_IW, 32, 2, 8),
    "vae": ("vae", 0, 128, 4, 1),
    "vae_gmp": ("vae_gmp", 0, 128, 4, 5),
}


@dataclasses.dataclass(frozen=True)
class SweepCase:
    id: str
    form: str
    model: str
    flags: int
    d: object           # oracle.Dims, S included
    B: int
    widths: str         # A | B
    nh: int

    def ranges(self, nsplit_small=NSPLIT_SMALL):
        return expected_ranges(self.model, self.d, self.B, self.flags, nsplit_small)

    @property
    def rows(self):
        return self.B * self.d.S * (self.d.K if self.flags & (OBJ_MARGINAL_Y | OBJ_MARGINAL_Y_IW) else 1)


SWEEP = []
for _form, (_model, _flags, _B, _S, _K) in FORMS.items():
    for _w, (_widths, _D) in WIDTHS.items():
        for _nh in range(1, MAX_HIDDEN + 1):
            SWEEP.append(SweepCase(f"{_form}-{_w}-nh{_nh}", _form, _model, _flags,
                                   O.Dims(D=_D, L=LATENT, K=_K, hidden=_widths[:_nh], S=_S), _B, _w, _nh))
SWEEP_BY_ID = {c.id: c for c in SWEEP}
assert len(SWEEP_BY_ID) == len(SWEEP) == 80

# The first site that is turned away, by depth (read off run_step_impl; tests/test_deep_networks_cpu.py holds expected_ranges to it)
FIRST_REFUSED = {
    "gmvae-gumbel": {1: None, 2: "encoder", 3: "layer0_y", 4: "encoder_gmm_upper", 5: "encoder_gmm_upper", 6: "encoder_gmm_upper",
                     7: "encoder_gmm_upper", 8: "decoder"},
    "vae": {1: None, 2: None, 3: None, 4: "encoder", 5: "encoder", 6: "encoder", 7: "encoder", 8: "decoder"},      # (nh = 8: 18 > 16)
}
FIRST_REFUSED["vae_gmp"] = FIRST_REFUSED["vae"]
# (D * hidden[0]) % 4 != 0 and the table full behind the x rows: the y rows' entry is dropped (the second with y summed out)
DROPPED_ENTRIES = ("gmvae-gumbel-B-nh3", "gmvae-marginal_iw-B-nh3")


# The many-splits count with no switch set: R = 6800 rows is the first size at which num_splits_small(R) = 17 exceeds NS = 16.
# (model, Dims, B): one sample per row (the x rows keep NS) and four (the x rows take num_splits(B) = 6), both with the ragged
# float4 between the x and the y rows of encoder_gmm's first layer (D * hidden[0] % 4 != 0)
THRESHOLD_CASES = [("gmvae", O.Dims(D=49, L=LATENT, K=5, hidden=(22, 12), S=1), 6800),
                   ("gmvae", O.Dims(D=49, L=LATENT, K=5, hidden=(22, 12), S=4), 1700)]


# ------------------------------------------------------------------------------ 3. middle layers on the row-panel paths
def per_row_forward_kernels(model, d, B, flags=0, planes_exact=False):
    """{(net, layer): kernel} of the hidden layers that run over all R rows in the forward pass (the decoder's below its top, the
    upper ones of encoder_gmm): rows_ws (rowsws.hpp, the weight stationary: 64 inputs, outputs % 64), rows_nn_bf6 (skinny.hpp:
    ReLU, R >= 2048, inputs % 32, outputs % 64) or gemm_grouped (gemm.hpp).  gmvae_step_profile names the LAUNCH ("fwd_dec",
    "fwd_enc_gmm") whichever of the three runs it: this restates the gates the names cannot tell apart.  (rws_fits' upper bound --
    at most 8 x the compute units of column slices -- is met by any width here.)"""
    marg = model == "gmvae" and bool(flags & (OBJ_MARGINAL_Y | OBJ_MARGINAL_Y_IW))
    R = B * d.S * (d.K if marg else 1)
    relu = d.act == "relu"
    rows_ok = lambda k, n: relu and R >= 2048 and k % 32 == 0 and n % 64 == 0
    rws_on = relu and R >= 2048
    out = {}
    dec = (d.L,) + tuple(d.hidden) + (d.D,)
    for i in range(len(d.hidden)):
        last_hidden_as_planes = planes_exact and i == len(d.hidden) - 1
        if rws_on and dec[i] == 64 and dec[i + 1] % 64 == 0 and not last_hidden_as_planes:
            out["decoder", i] = "rows_ws"
        else:
            out["decoder", i] = "rows_nn_bf6" if rows_ok(dec[i], dec[i + 1]) else "gemm_grouped"
    if model == "gmvae":
        g = (d.D + d.K,) + tuple(d.hidden) + (2 * d.L,)
        for i in range(1, len(d.hidden) + 1):
            out["encoder_gmm", i] = "rows_nn_bf6" if rows_ok(g[i], g[i + 1]) else "gemm_grouped"
    return out


@dataclasses.dataclass(frozen=True)
class PanelCase:
    id: str
    model: str
    d: object
    B: int
    plane_rows: bool            # R % 128 == 0: the plane launches are eligible by their row count (their own size gates still decide)
    names: tuple                # gmvae_step_profile's names, in launch order


# One launch per layer and per head (eps and u fed: no noise launch; S = 1: no sum_over_s; hidden[0] % 64 == 0 and D % 16 == 0: the
# first layers over x in first_layers_u8bf).  The one name that tells a kernel: bwd_enc_gmm_dh, the data gradient of encoder_gmm's
# MIDDLE layer (64 -> 128 forward, so 128 -> 64 backward) in rows_ws behind that layer's weight-gradient launch.
_GM_NAMES = (("fwd_x_first_layers",) + 3 * ("fwd_enc_y",) + ("y_head_fwd", "fwd_y_layers") + 3 * ("fwd_enc_gmm",) + ("z_head_fwd",)
             + 3 * ("fwd_dec",) + ("fwd_dec_bernoulli", "row_terms", "loss_tail", "bwd_dec_top") + 3 * ("bwd_dec",) + ("z_head_bwd",)
             + 3 * ("bwd_enc_gmm",) + ("bwd_enc_gmm_dh", "bwd_enc_gmm_l0", "y_head_bwd") + 3 * ("bwd_enc",)
             + ("bwd_enc_l0", "finalize_grads"))
_VAE_NAMES = (("fwd_x_first_layers",) + 4 * ("fwd_enc",) + ("z_head_fwd",) + 4 * ("fwd_dec",)
              + ("fwd_dec_bernoulli", "row_terms", "loss_tail", "bwd_dec_top") + 4 * ("bwd_dec",) + ("z_head_bwd",) + 4 * ("bwd_enc",)
              + ("bwd_enc_l0", "finalize_grads"))
PANEL_CASES = [
    PanelCase("gmvae-h64x128x64-B2112", "gmvae", O.Dims(D=256, L=32, K=32, hidden=(64, 128, 64)), 2112, False, _GM_NAMES),
    PanelCase("gmvae-h64x128x64-B2176", "gmvae", O.Dims(D=256, L=32, K=32, hidden=(64, 128, 64)), 2176, True, _GM_NAMES),
    PanelCase("vae-h128x64x128x64-B2112", "vae", O.Dims(D=256, L=32, K=1, hidden=(128, 64, 128, 64)), 2112, False, _VAE_NAMES),
]

# ------------------------------------------------------------------------------- 4. depth under every objective family
FAMILY_DIMS = dict(D=100, L=5, K=4, hidden=(24, 16, 20, 12))
FAMILY_B = 9

# ------------------------------------------------------------------------------------- 5. eight hidden layers end to end
EIGHT = dict(D=48, L=LATENT, K=5, hidden=WIDTHS["A"][0])
EIGHT_B = 10
