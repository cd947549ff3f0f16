"""The corners of the step schedules' size gates (csrc/gmvae_hip.hip: mega_shape, mega2_ok, mega2v_kind / mega2v_ok, fused_shape,
skinny_shape, evalf_shape / evalf_ok) -- test infrastructure, a plain module: one table for tests/test_gate_corners_cpu.py (the
table against the predicates, no device) and tests/test_gate_corners.py (every corner against the fp64 oracle on the device).

Every corner is derived from the predicates as they stand: the last shape a gate admits (or the first one a kernel's compile-time
constant treats differently -- mega.hpp kCW = 128 and kFlLda = 226, aux.hpp kMaxImgTasks = 32, the 160 KB / 156 KB LDS budgets,
GMP_PARTS = 64, kSkMaxB = 4096, the 16-lane softmax behind K <= 16, evalf.hpp EV::NB = 8, ceil(B / kPanel) * 7 <= 256) and, where
`outside_of` names a corner, the
first shape past that corner's gate, which must fall to ANOTHER schedule and still match.  Dimensions that are not under test stay
small (D = 64 or 128, one ragged pair of panels).  A change of a gate constant fails tests/test_gate_corners_cpu.py first: move
the corner to the new edge and keep the old shape as the `outside_of` case.

kind   step   one eager training step: hip_util.compare_step at test_step_matches_oracle's preparation
       evalf  forward only: gmvae_forward's rows and tail against oracle.forward
       train  three steps of a train graph: test_timed_path.trajectory_case
sched  the leading word of gmvae_step_schedule under `env` ("evalf" / "other" for the forward-only corners, which that entry point
       does not name: the device test tells them apart by the bits of GMVAE_NO_EVALF=1's rows)
edge   the batch follows the device's compute-unit count as the predicate reads it (batch_on); B is its value at 256 units"""
import dataclasses

import oracle as O

SWITCHES = ("GMVAE_NO_MEGA", "GMVAE_NO_FUSED", "GMVAE_NO_MEGA2", "GMVAE_NO_SKINNY", "GMVAE_NO_EVALF")
PANEL = 16            # chain.hpp kPanel
EV_NB = 8             # evalf.hpp EV::NB
GMP_PARTS = 64
SK_MAX_B = 4096       # kSkMaxB


@dataclasses.dataclass(frozen=True)
class Corner:
    id: str
    kind: str
    model: str
    d: object                  # oracle.Dims
    B: int
    env: tuple                 # ((switch, value), ...)
    sched: str
    outside_of: str = None     # id of the corner whose gate this shape is the first one past
    edge: str = None           # evalf | mega2v: see batch_on
    fl_inside: int = None      # train corners on `mega`: whether steps 2..n run the first layer inside the launch (mega_lay fl_ok)


def batch_on(c, cus):
    """The corner's batch on a device of `cus` compute units."""
    if c.edge == "evalf":          # evalf_ok at S = 1: grid = min(cus, B, 1024) workgroups of at most EV::NB batch rows
        return min(cus, 1024) * EV_NB + (1 if c.outside_of else 0)
    if c.edge == "mega2v":         # mega2v_kind: ceil(B / kPanel) * 7 <= 256; mega2v_ok: ... <= cus
        return min(cus, 256) // 7 * PANEL + (1 if c.outside_of else 0)
    return c.B


FUSED = (("GMVAE_NO_MEGA", "1"), ("GMVAE_NO_SKINNY", "1"))       # gmvae_step_schedule asks skinny_ok before fused_ok
SKINNY = (("GMVAE_NO_MEGA", "1"), ("GMVAE_NO_FUSED", "1"))
KDEF = {"gmvae": 10, "vae": 1, "vae_gmp": 10}
MODELS = ("gmvae", "vae", "vae_gmp")

MEGA_DMAX = {"gmvae": 1280, "vae": 1664, "vae_gmp": 1536}        # 10 / 13 / 12 decoder chunks of kCW = 128 columns

CORNERS = []


def _add(id, kind, model, B, env, sched, outside_of=None, edge=None, fl_inside=None, **dims):
    dims.setdefault("K", KDEF[model])
    H = dims.pop("H", 64)
    CORNERS.append(Corner(id, kind, model, O.Dims(hidden=(H,), **dims), B, env, sched, outside_of, edge, fl_inside))


# ------------------------------------------------------------------------------------------------------------------ mega
for m in MODELS:
    _add(f"mega-{m}-D16", "step", m, 24, (), "mega", D=16, L=8)             # one decoder chunk, narrower than kCW
    _add(f"mega-{m}-D896", "step", m, 24, (), "mega", D=896, L=8)           # the last D with fl_kq = 224 <= kFlLda
    _add(f"mega-{m}-D912", "step", m, 24, (), "mega", D=912, L=8)           # the first with fl_kq = 228: mega_lay fl_ok false
    # the last D whose image tasks -- the small-weight image's tensors + two per decoder chunk -- fit aux.hpp kMaxImgTasks = 32
    # (mega_img_tasks), the first one past it, and D = 3072 (24 chunks), which mega_shape admitted until these corners ran
    _add(f"mega-{m}-D{MEGA_DMAX[m]}", "step", m, 24, (), "mega", D=MEGA_DMAX[m], L=8)
    _add(f"mega-{m}-D{MEGA_DMAX[m] + 16}", "step", m, 24, (), "skinny", f"mega-{m}-D{MEGA_DMAX[m]}", D=MEGA_DMAX[m] + 16, L=8)
    _add(f"mega-{m}-D3072", "step", m, 24, (), "skinny", f"mega-{m}-D{MEGA_DMAX[m]}", D=3072, L=8)
    _add(f"mega-{m}-H16", "step", m, 24, (), "mega", D=128, L=8, H=16)
    _add(f"mega-{m}-L2", "step", m, 24, (), "mega", D=128, L=2)
    for B in (1, PANEL - 1, PANEL + 1):
        _add(f"mega-{m}-B{B}", "step", m, B, (), "mega", D=64, L=8)
# L = 128 fits the 160 KB budget at H = 16 alone, up to K = 16 (GMVAE) / K = 7 (VAE_GMP): both are LDS edges too
_add("mega-gmvae-L128", "step", "gmvae", 24, (), "mega", D=128, L=128, K=16, H=16)
_add("mega-gmvae-L128-K17", "step", "gmvae", 24, (), "general", "mega-gmvae-L128", D=128, L=128, K=17, H=16)
_add("mega-vae-L128", "step", "vae", 24, (), "mega", D=128, L=128, H=16)
_add("mega-vae_gmp-L128", "step", "vae_gmp", 24, (), "mega", D=128, L=128, K=7, H=16)
_add("mega-vae_gmp-L128-K8", "step", "vae_gmp", 24, (), "general", "mega-vae_gmp-L128", D=128, L=128, K=8, H=16)
for m in ("gmvae", "vae_gmp"):
    for K in (1, 33, 64):
        _add(f"mega-{m}-K{K}", "step", m, 24, (), "mega", D=128, L=8, K=K)
_add("mega-gmvae-K65", "step", "gmvae", 24, (), "general", "mega-gmvae-K64", D=128, L=8, K=65)
# VAE_GMP: one prior-gradient partial per panel, GMP_PARTS of them
_add("mega-vae_gmp-panels64", "step", "vae_gmp", GMP_PARTS * PANEL, (), "mega", D=64, L=8)
_add("mega-vae_gmp-panels65", "step", "vae_gmp", GMP_PARTS * PANEL + 1, (), "skinny", "mega-vae_gmp-panels64", D=64, L=8)
# H = 64: the admitted (L, K) with the largest mega_lay(...).total * 4 (searched over every even L <= 128 and K <= 64; bytes in
# profiles/gate_corners_notes.md) and its nearest rejected neighbour
_add("mega-gmvae-lds-edge", "step", "gmvae", 24, (), "mega", D=128, L=38, K=55)              # 163,840 B = the budget itself
_add("mega-gmvae-lds-over", "step", "gmvae", 24, (), "general", "mega-gmvae-lds-edge", D=128, L=38, K=56)
_add("mega-vae-lds-edge", "step", "vae", 24, (), "mega", D=128, L=76)                        # 160,528 B
_add("mega-vae-lds-over", "step", "vae", 24, (), "general", "mega-vae-lds-edge", D=128, L=78)
_add("mega-vae_gmp-lds-edge", "step", "vae_gmp", 24, (), "mega", D=128, L=36, K=39)          # 163,776 B
_add("mega-vae_gmp-lds-over", "step", "vae_gmp", 24, (), "skinny", "mega-vae_gmp-lds-edge", D=128, L=36, K=40)

# ----------------------------------------------------------------------------------------------------------------- fused
_add("fused-L8", "step", "gmvae", 24, FUSED, "fused", D=128, L=8)
_add("fused-L12", "step", "gmvae", 24, FUSED, "general", "fused-L8", D=128, L=12)            # L % 8 != 0
_add("fused-L128", "step", "gmvae", 24, FUSED, "fused", D=128, L=128, K=16, H=16)            # (H = 16, K <= 16: the 156 KB budget)
_add("fused-L128-K17", "step", "gmvae", 24, FUSED, "general", "fused-L128", D=128, L=128, K=17, H=16)
_add("fused-K64", "step", "gmvae", 24, FUSED, "fused", D=128, L=8, K=64)
_add("fused-H16", "step", "gmvae", 24, FUSED, "fused", D=128, L=8, H=16)
# H = 64: the admitted (L, K) with the largest max(fwd_lay, bwd_lay).total * 4: 159,712 B of 159,744
_add("fused-lds-edge", "step", "gmvae", 24, FUSED, "fused", D=128, L=64, K=23)
_add("fused-lds-over", "step", "gmvae", 24, FUSED, "general", "fused-lds-edge", D=128, L=64, K=24)

# ---------------------------------------------------------------------------------------------------------------- skinny
for m in MODELS:
    _add(f"skinny-{m}-D16", "step", m, 24, SKINNY, "skinny", D=16, L=8)
    _add(f"skinny-{m}-D3072", "step", m, 24, SKINNY, "skinny", D=3072, L=8)
    _add(f"skinny-{m}-L4", "step", m, 24, SKINNY, "skinny", D=64, L=4)
    _add(f"skinny-{m}-L256", "step", m, 24, SKINNY, "skinny", D=64, L=256)
    _add(f"skinny-{m}-L260", "step", m, 24, SKINNY, "general", f"skinny-{m}-L256", D=64, L=260)
_add("skinny-H64", "step", "gmvae", 24, SKINNY, "skinny", D=128, L=8)
_add("skinny-H1024", "step", "gmvae", 24, SKINNY, "skinny", D=64, L=8, H=1024)
_add("skinny-H1088", "step", "gmvae", 24, SKINNY, "general", "skinny-H1024", D=64, L=8, H=1088)
_add("skinny-K16", "step", "gmvae", 24, SKINNY, "skinny", D=64, L=8, K=16)
_add("skinny-K17", "step", "gmvae", 24, SKINNY, "general", "skinny-K16", D=64, L=8, K=17)
for B in (1, 128, 129):                                                  # (the forms for more than 128 rows start at 129)
    _add(f"skinny-B{B}", "step", "gmvae", B, SKINNY, "skinny", D=64, L=8)
_add("skinny-B4096", "step", "gmvae", SK_MAX_B, SKINNY, "skinny", D=64, L=8)
_add("skinny-B4097", "step", "gmvae", SK_MAX_B + 1, SKINNY, "general", "skinny-B4096", D=64, L=8)

# ----------------------------------------------------------------------------------------------------------------- evalf
for m, L in (("gmvae", 64), ("vae", 2), ("vae_gmp", 64)):
    _add(f"evalf-{m}-NB", "evalf", m, 256 * EV_NB, (), "evalf", edge="evalf", D=784, L=L)
    _add(f"evalf-{m}-NB+1", "evalf", m, 256 * EV_NB + 1, (), "other", f"evalf-{m}-NB", edge="evalf", D=784, L=L)

# --------------------------------------------------------------------------------- the training path (mega2/3, mega2v/3v)
for B in (1, 1023, 1024):
    _add(f"train-gmvae-B{B}", "train", "gmvae", B, (), "mega2", D=784, L=64)
_add("train-gmvae-B1025", "train", "gmvae", 1025, (), "mega", "train-gmvae-B1024", D=784, L=64)
for m, L in (("vae", 2), ("vae_gmp", 64)):
    _add(f"train-{m}-panels36", "train", m, 576, (), "mega2v", edge="mega2v", D=784, L=L)
    _add(f"train-{m}-panels37", "train", m, 577, (), "mega", f"train-{m}-panels36", edge="mega2v", D=784, L=L)
# the in-launch first layer (a train graph only: an eager step never runs it) at the last D its x image holds (fl_kq = 224 <=
# kFlLda) and at the first one past it.  mega_lay's fl_ok also wants the first-layer staging -- 2 x fl_kq x H floats for the GMVAE
# -- below the row-sum scratch: at D = 896, K = 10 that holds from L = 36 (16 floats to spare), and L = 34 is its first miss
_add("train-gmvae-D896", "train", "gmvae", 96, (), "mega", D=896, L=36, fl_inside=1)
_add("train-gmvae-D912", "train", "gmvae", 96, (), "mega", D=912, L=36, fl_inside=0)
_add("train-gmvae-D896-L34", "train", "gmvae", 96, (), "mega", D=896, L=34, fl_inside=0)
# (the VAE family stages one first-layer tensor: the staging fits at any latent size; mega2v takes D = 784 alone)
for m in ("vae", "vae_gmp"):
    _add(f"train-{m}-D896", "train", m, 96, (), "mega", D=896, L=8, fl_inside=1)
    _add(f"train-{m}-D912", "train", m, 96, (), "mega", D=912, L=8, fl_inside=0)

BY_ID = {c.id: c for c in CORNERS}
assert len(BY_ID) == len(CORNERS)
