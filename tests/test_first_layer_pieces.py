"""The in-launch first layer of the GMVAE step (csrc/mega2.hpp `FL:`, shared by mega2_fwd_bwd and mega3_step) on exact bf16 piece
products (csrc/bf16x3.hpp): the batch bytes are exact in bf16, each fp32 weight is hi + mid + lo bf16 pieces, every product is
exact and the fp32 accumulation is the only rounding.

The block runs where the optimizer owns the weight images, i.e. in a train-graph step (a plain gmvae_step takes its first layer
from a launch of its own), so the steps here are one-step train graphs of an Engine; step 0 of a graph builds the images from
the parameters it is given.  The kept activations are read from the workspace by name ("hy1", "hg1"), GMVAE 784-64-64-10, S = 1.
Batches: 16 (the pair's second panel is a phantom), 32 (one full pair), 48 (two pairs, the last panel a phantom), 40 (a ragged
last panel), 1024 (the only size that runs mega3_step by itself).

Measured on MI355X (dense pairing, max |device - fp64| as a fraction of the accumulation bound): see
profiles/first_layer_pieces_notes.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

D, H, LZ, K = 784, 64, 64, 10
DIMS = O.Dims(D=D, L=LZ, K=K, hidden=(H,))
WY, WG = "encoder_y_fcnet/linear_0/w", "encoder_gmm_fcnet/linear_0/w"
BATCHES = (16, 32, 48, 40, 1024)
# both ends of every quarter (196 columns each) and of every block of 32 contraction steps inside one
TAPS = (0, 31, 32, 191, 192, 195, 196, 391, 392, 587, 588, 779, 783)
_ENGINES = {}


def _engine(B, form=""):
    """One engine and one-step train graph per (batch, launch form): (engine, static x, replay)."""
    from gmvae_amd.engine import Engine
    if (B, form) not in _ENGINES:
        e = Engine("gmvae", D, LZ, K, [H], random_seed=7)
        sx, replay = e.capture_train_step(B, 1e-3, n_steps=1)
        _ENGINES[(B, form)] = (e, sx, replay)
    return _ENGINES[(B, form)]


def _first_layer(B, params, x, form=""):
    """hy1, hg1 [B, 64] (float32 numpy) of ONE train step on batch x from the parameters `params` (name -> array), and the step's
    launch names."""
    from gmvae_amd import _lib as L
    e, sx, replay = _engine(B, form)
    flat = O.pack(O.MODEL_GMVAE, DIMS, params, np.float32)
    assert flat.size == e.P
    with torch.no_grad():
        e.params.copy_(torch.from_numpy(flat))
    sx.copy_(torch.from_numpy(x))
    replay()
    torch.cuda.synchronize()
    assert e.handoff_timeouts() == 0
    d, ws = e._workspace(B)
    out = []
    for name in (b"hy1", b"hg1"):
        off = C.c_uint64()
        L.check(L.lib.gmvae_workspace_offset(C.byref(d), e.model, name, C.byref(off)), "offset " + name.decode())
        out.append(ws[off.value // 4: off.value // 4 + B * H].view(B, H).cpu().numpy().copy())
    names = [nm for nm, _, _, _ in e.profile_train_levels(torch.from_numpy(x).cuda(), iters=2)]
    return out[0], out[1], names


def _full_weights(rng, shape):
    """fp32 with full 24-bit significands (the lowest bit set: all three pieces are non-zero), both signs, |w| in [2^-12, 1)."""
    mant = (rng.integers(0, 1 << 23, size=shape, dtype=np.int64) | 1).astype(np.float64) / float(1 << 23)
    w = (1.0 + mant) * np.exp2(rng.integers(-12, 0, size=shape).astype(np.float64)) * rng.choice([-1.0, 1.0], size=shape)
    w32 = w.astype(np.float32)
    assert (w32.astype(np.float64) == w).all()
    return w32


def _params(rng, wy, wg):
    """Xavier everywhere but the two first layers: weights wy / wg over the x rows, zero biases, zero y rows of encoder_gmm's."""
    p = O.init_params(O.MODEL_GMVAE, DIMS, rng, np.float32)
    p[WY] = wy
    p[WG] = np.concatenate([wg, np.zeros((K, H), np.float32)], axis=0)
    for net in ("encoder_y", "encoder_gmm"):
        p[f"{net}_fcnet/linear_0/b"] = np.zeros(H, np.float32)
    return p


def _launches(B, names, form=""):
    one = form == "fuse" or (form == "" and B == 1024)
    assert names == (["mega3_step"] if one else ["mega2_fwd_bwd", "dw_adam"]), names


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("B", BATCHES)
def test_single_tap_is_exact_bit_for_bit(B):
    """Every batch row has ONE non-zero pixel, at column k_r: hy1[r][n] = max(0, x_r Wy0[k_r][n]) and hg1 likewise -- the other
    quarters and taps contribute exact zeros -- and x_r w is exact in fp32 in both variants, so the device must give the bits of
    numpy's fp32 product.  (a) pixels = the powers of two 1..128, weights with full 24-bit significands; (b) pixels = every byte
    value (37 r + B mod 256 over the rows: all 256 at B = 1024), weights rounded to 16 significant bits.  Each with W and -W, so
    both signs pass the ReLU.  A dropped or misplaced piece and any wrong contraction index shows here."""
    rng = np.random.default_rng(1000 + B)
    rows = np.arange(B)
    cols = rng.integers(0, D, size=B)
    cols[:len(TAPS)] = TAPS
    if B > 2 * len(TAPS):
        cols[B - len(TAPS):] = TAPS                # the last (ragged / second row tile's) rows take them too
    for variant in ("a", "b"):
        if variant == "a":
            vals = (1 << (rows % 8)).astype(np.uint8)
            wy, wg = _full_weights(rng, (D, H)), _full_weights(rng, (D, H))
        else:
            vals = ((37 * rows + B) % 256).astype(np.uint8)
            wy = (_bits(_full_weights(rng, (D, H))) & np.uint32(0xFFFFFF00)).view(np.float32)
            wg = (_bits(_full_weights(rng, (D, H))) & np.uint32(0xFFFFFF00)).view(np.float32)
        x = np.zeros((B, D), np.uint8)
        x[rows, cols] = vals
        for sign in (1.0, -1.0):
            sy, sg = np.float32(sign) * wy, np.float32(sign) * wg
            hy, hg, names = _first_layer(B, _params(rng, sy, sg), x)
            _launches(B, names)
            for what, got, w in (("hy1", hy, sy), ("hg1", hg, sg)):
                prod = vals.astype(np.float32)[:, None] * w[cols]            # fp32 multiplies: exact by construction
                assert (prod.astype(np.float64) == vals.astype(np.float64)[:, None] * w[cols].astype(np.float64)).all()
                want = np.where(prod > 0, prod, np.float32(0))
                bad = _bits(got) != _bits(want)
                assert not bad.any(), (f"B = {B} variant ({variant}) sign {sign:+.0f} {what}: {int(bad.sum())} of {bad.size} differ; first at "
                                       f"(row, column) {tuple(np.argwhere(bad)[0])}, tap column {cols[np.argwhere(bad)[0][0]]}: "
                                       f"{got[bad][0]!r} != {want[bad][0]!r}")


@pytest.mark.parametrize("B", (32, 40))
def test_dense_rows_stay_inside_the_accumulation_bound(B):
    """Random bytes over 0..255 against full-significand weights, zero biases: hy1 and hg1 against an fp64 evaluation, within the
    accumulation's own bound per element, (3 x 224 + 3) 2^-24 sum_k |x_k w_k| + 2^-24 |ref| (3 x 224 piece products accumulated
    per quarter, 3 quarter sums, the final rounding).  An A / B contraction mismatch across taps shows here."""
    rng = np.random.default_rng(2000 + B)
    x = rng.integers(0, 256, size=(B, D), dtype=np.uint8)
    wy, wg = _full_weights(rng, (D, H)), _full_weights(rng, (D, H))
    hy, hg, names = _first_layer(B, _params(rng, wy, wg), x)
    _launches(B, names)
    xf = x.astype(np.float64)
    for what, got, w in (("hy1", hy, wy), ("hg1", hg, wg)):
        ref = xf @ w.astype(np.float64)
        bound = (3 * 224 + 3) * 2.0 ** -24 * (xf @ np.abs(w.astype(np.float64))) + 2.0 ** -24 * np.abs(ref)
        err = np.abs(got.astype(np.float64) - np.maximum(ref, 0))
        print(f"B = {B} {what}: max |device - fp64| / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("B", (1024, 40))
def test_the_two_launch_forms_keep_the_same_first_layer(B, monkeypatch):
    """hy1 and hg1 of a step as mega3_step (GMVAE_FUSE=1; B = 1024 takes it by itself) equal those as mega2_fwd_bwd -> dw_adam
    (GMVAE_NO_FUSE=1) bit for bit: one body, no launch-dependent arithmetic."""
    rng = np.random.default_rng(3000 + B)
    x = rng.integers(0, 256, size=(B, D), dtype=np.uint8)
    p = _params(rng, _full_weights(rng, (D, H)), _full_weights(rng, (D, H)))
    res = {}
    for form in ("fuse", "nofuse"):
        if form == "fuse":
            monkeypatch.delenv("GMVAE_NO_FUSE", raising=False); monkeypatch.setenv("GMVAE_FUSE", "1")
        else:
            monkeypatch.setenv("GMVAE_NO_FUSE", "1"); monkeypatch.delenv("GMVAE_FUSE", raising=False)
        hy, hg, names = _first_layer(B, p, x, form)
        _launches(B, names, form)
        res[form] = (hy, hg)
    for a, b, what in zip(res["fuse"], res["nofuse"], ("hy1", "hg1")):
        assert np.isfinite(a).all() and (a > 0).any() and (_bits(a) == _bits(b)).all(), what
