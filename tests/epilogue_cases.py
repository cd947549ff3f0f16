"""The top decoder layer's loss epilogues (csrc/gemm.hpp gemm_grouped: EPI_BERNOULLI under GMVAE_OBJ_PIXEL_MASK, EPI_LIK and its
LIK_XF32 / LIK_RHO forms) x the tile configurations x the code paths inside a tile -- test infrastructure, a plain module: one
table for tests/test_epilogue_forms_cpu.py (the table against a restatement of the tile classification, no device) and
tests/test_epilogue_forms.py (every entry against its family's fp64 statement on the device).

A tile of the logits launch [R, D] under a configuration of BM x BN takes one of four paths (gemm.hpp: `tile_ok` of EPI_LIK, the
same condition in front of EPI_BERNOULLI's interior block):
    unaligned   D % 4 != 0 (ldc & 3): every tile goes element by element, with scalar stores
    ragged      m0 + BM > R: element by element (rows beyond R skipped, 16-byte stores where a quad is whole)
    quad        m0 + BM <= R, n0 + BN > D, D % 4 == 0: the interior block with the column quads beyond D predicated off
    interior    m0 + BM <= R and n0 + BN <= D
The shapes are the smallest that put every path into every configuration (tests/test_epilogue_forms_cpu.py asserts it):
    whole      R = 32 x 4 = 128, D = 256, H = 128: under 128 x 128 every tile is interior and the launch takes the big-round
               instance (gmvae_hip.hip big_eligible: M % 128 == 0, N % 128 == 0, K % 32 == 0); the IWAE row weights are live
    ragged     R = 168 = 128 + 40 = 2 x 64 + 40 = 5 x 32 + 8, D = 272 = 2 x 128 + 16 = 4 x 64 + 16 = 8 x 32 + 16: interior tiles,
               the quad-predicated last column tile and ragged-row tiles under all three (R = 160 has no ragged row at 32 x 32)
    unaligned  R = 70, D = 135: the element path's row butterfly 8, 16 or 32 lanes wide"""
import dataclasses

import numpy as np

import lik_ref as LR
import oracle as O
import pmask_ref as PR
import realx_ref as RR

OBJ_PIXEL_MASK = 512                                        # include/gmvae_hip.h GMVAE_OBJ_PIXEL_MASK
TILE = {0: (32, 32), 1: (64, 64), 2: (128, 128)}            # GMVAE_FORCE_CFG -> (BM, BN): gemm.hpp CfgS, CfgM, CfgL
CFGS = (0, 1, 2)
PATHS = ("interior", "quad", "ragged", "unaligned")
SIGMA = 0.25                                                # the fixed-scale Gaussians' sigma (lik_ref's and realx_ref's own)


@dataclasses.dataclass(frozen=True)
class Family:
    kind: str            # the fp64 statement: mask -> pmask_ref, lik -> lik_ref, realx -> realx_ref
    flags: int
    lik: str = None      # lik_ref's name of the likelihood
    f32: bool = False    # x as float32 (GMVAE_X_F32)
    learned: bool = False


FAMILIES = {
    "mask": Family("mask", OBJ_PIXEL_MASK),
    "grey": Family("lik", LR.FLAG["grey"], "grey"),
    "cb": Family("lik", LR.FLAG["cb"], "cb"),
    "gauss": Family("lik", LR.FLAG["gauss"], "gauss"),
    "gauss-f32": Family("realx", RR.LIK_GAUSSIAN | RR.X_F32, f32=True),
    "gauss-lsig": Family("realx", RR.LIK_GAUSSIAN | RR.LIK_SCALE_LEARNED, learned=True),
    "gauss-f32-lsig": Family("realx", RR.LIK_GAUSSIAN | RR.X_F32 | RR.LIK_SCALE_LEARNED, f32=True, learned=True),
}


@dataclasses.dataclass(frozen=True)
class Shape:
    mname: str
    d: object
    B: int


SHAPES = {
    "whole": Shape("gmvae", O.Dims(D=256, L=64, K=10, hidden=(128,), S=4), 32),
    "ragged": Shape("gmvae", O.Dims(D=272, L=8, K=7, hidden=(64,)), 168),
    "unaligned": Shape("gmvae", O.Dims(D=135, L=5, K=7, hidden=(24,)), 70),
    # "ragged" once more per other model, for the two families with the learned scale on real-valued layouts
    "ragged-vae": Shape("vae", O.Dims(D=272, L=8, K=1, hidden=(64,)), 168),
    "ragged-vae_gmp-tanh": Shape("vae_gmp", O.Dims(D=272, L=8, K=7, hidden=(64,), act="tanh"), 168),
}
OTHER_MODELS = ("ragged-vae", "ragged-vae_gmp-tanh")
# (family, shape) of every step case; tests/test_epilogue_forms.py runs each under GMVAE_FORCE_CFG = 0, 1, 2
STEP_CASES = [(f, s) for f in FAMILIES for s in ("whole", "ragged", "unaligned")] + \
             [(f, s) for f in ("gauss-lsig", "gauss-f32-lsig") for s in OTHER_MODELS]
# gmvae_forward (no C output: the `Cout == nullptr` instantiations) under GMVAE_FORCE_CFG = 1, 2
FORWARD_CASES = [("mask", "ragged"), ("cb", "ragged"), ("gauss-f32-lsig", "ragged")]
FORWARD_CFGS = (1, 2)


def tile_paths(R, D, BM, BN):
    """The set of paths the tiles of a [R, D] logits launch take under BM x BN tiles."""
    if D % 4:
        return {"unaligned"}
    out = set()
    for m0 in range(0, R, BM):
        for n0 in range(0, D, BN):
            out.add("ragged" if m0 + BM > R else ("interior" if n0 + BN <= D else "quad"))
    return out


def big_round_eligible(R, D, H):
    """gmvae_hip.hip big_eligible for the logits launch [R, D] over H: whole 128 x 128 tiles, whole 32-deep rounds."""
    return R % 128 == 0 and D % 128 == 0 and H % 32 == 0


@dataclasses.dataclass
class Inputs:
    family: str
    shape: str
    model: int
    d: object
    B: int
    p32: dict
    flat: np.ndarray        # the parameters as the device takes them (rho appended under the learned scale)
    x: np.ndarray           # as the device takes it: uint8 or float32
    eps: np.ndarray
    u: object
    flags: int
    regions: dict           # hip_util.write_inputs' mapping: the caller-written workspace regions
    mask: object = None     # mask family: the observation mask
    t: object = None        # realx families: the targets, float64
    rho: object = None      # float64 [D] under the learned scale


def build(family, shape):
    """The inputs of one case: parameters Xavier with biases N(0, 0.05) (test_memory_contract._corner_inputs' preparation), the
    noise of oracle.make_inputs, and the family's own batch -- binary x flipped at the missing pixels of pmask_ref.make_mask;
    lik_ref.grey_batch; realx_ref.real_batch (x and rho)."""
    fam, sh = FAMILIES[family], SHAPES[shape]
    model, d, B = O.MODEL_NAMES[sh.mname], sh.d, sh.B
    rng = np.random.default_rng(B)
    p = O.init_params(model, d, rng)
    for k in p:
        if k.endswith("/b"):
            p[k] = rng.normal(0, 0.05, p[k].shape)
    xb, eps, u = O.make_inputs(d, B, model)
    u = u if model == O.MODEL_GMVAE else None
    flat = O.pack(model, d, p, np.float32)
    p32 = O.unpack(model, d, flat.astype(np.float64))
    I = Inputs(family, shape, model, d, B, p32, flat, None, eps, u, fam.flags, {})
    if fam.kind == "mask":
        I.mask = PR.make_mask(B, d.D)
        I.x = PR.flip_missing(xb, I.mask)
        I.regions = {"pixel_mask": I.mask}
    elif fam.kind == "lik":
        I.x = LR.grey_batch(B, d.D)
        if fam.lik == "gauss":
            I.regions = {"lik_sigma": np.array([SIGMA], np.float32)}
    else:
        xf, rho32 = RR.real_batch(B, d.D)
        if fam.f32:
            I.x, I.t = xf, xf.astype(np.float64)
        else:
            I.x = LR.grey_batch(B, d.D)
            I.t = LR.targets(I.x)
        if fam.learned:
            tailp = np.zeros(RR.pad4(d.D), np.float32)
            tailp[:d.D] = rho32
            I.flat = np.concatenate([flat, tailp])
            I.rho = rho32.astype(np.float64)
        else:
            I.regions = {"lik_sigma": np.array([SIGMA], np.float32)}
    return I


def statement(I, relu_masks=None):
    """(C, g) of the family's fp64 statement on the case's inputs."""
    fam = FAMILIES[I.family]
    if fam.kind == "mask":
        return PR.loss_and_grads(I.model, I.d, I.p32, I.x, I.eps, I.u, I.mask, relu_masks=relu_masks)
    if fam.kind == "lik":
        return LR.loss_and_grads(I.model, I.d, I.p32, I.x, I.eps, I.u, fam.lik, SIGMA, relu_masks=relu_masks)
    return RR.loss_and_grads(I.model, I.d, I.p32, I.t, I.eps, I.u, sigma=SIGMA, rho=I.rho, relu_masks=relu_masks)


_CASES = {}      # (family, shape) -> (Inputs, (C, g)): built once, shared, left unchanged


def case(family, shape):
    if (family, shape) not in _CASES:
        I = build(family, shape)
        _CASES[(family, shape)] = (I, statement(I))
    return _CASES[(family, shape)]
