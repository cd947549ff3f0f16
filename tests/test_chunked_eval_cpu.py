"""CPU-side checks of what include/gmvae_hip.h documents for the four chunked importance-sampling evaluators together
(gmvae_iw_bound, gmvae_iw_bound_enum_y, gmvae_posterior_y, gmvae_posterior_component): how their workspace sizes relate, which
bits of sched_flags their size queries ignore, and the code of every failing argument, in the documented order of the checks
(dims, then NULL, then the range of n_samples, then alignment) and before any launch.  No compute calls."""
import ctypes as C
import itertools

import pytest


KINDS = ("iw_bound", "iw_bound_enum_y", "posterior_y", "posterior_component")
ENUM_Y = ("iw_bound_enum_y", "posterior_y")            # y summed out: GMVAE only, the marginal bits ignored
E_NULL, E_DIMS, E_MODEL, E_ALIGN = -1, -2, -3, -4
SHAPES = [      # (D, L, K, hidden): general-schedule shapes, the default sizes of csrc/evalf.hpp (L = 64 and 2), a wide layer, K > 64
    (100, 5, 7, (24, 24)), (784, 64, 10, (64,)), (784, 2, 1, (64,)), (60, 3, 4, (16,)), (784, 128, 10, (512,)), (100, 8, 80, (24,))]
BATCHES = [(1, 1), (8, 5), (5, 37), (64, 50)]          # (B, chunk)


@pytest.fixture(scope="module")
def L():
    import build_hip
    build_hip.build(verbose=False)
    from gmvae_amd import _lib
    return _lib


def maskable(L):
    """Every combination of the bits the four evaluators mask off."""
    bits = (L.SCHED_EVAL_IMAGES_VALID, L.GRAD_DREG, L.OBJ_LABELS, L.OBJ_WEIGHTS)
    return [sum(c) for r in range(len(bits) + 1) for c in itertools.combinations(bits, r)]


def marginal(L):
    return (0, L.OBJ_MARGINAL_Y, L.OBJ_MARGINAL_Y_IW, L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW)


def dims(L, shape, B, chunk, flags=0, row0=0):
    D, Lz, K, hidden = shape
    d = L.make_dims(B, D, Lz, K, hidden, S=chunk, sched_flags=flags)
    d.row0 = row0
    return d


def query(L, kind, d, model):
    """(return code, bytes) of gmvae_<kind>_workspace_bytes."""
    b = C.c_uint64()
    rc = getattr(L.lib, f"gmvae_{kind}_workspace_bytes")(C.byref(d), model, C.byref(b))
    return rc, b.value


def size_grid(L):
    """(shape, B, chunk, flags) over SHAPES x BATCHES x every maskable combination x the marginal bits."""
    return [(s, B, c, m | y) for s in SHAPES for B, c in BATCHES for m in maskable(L) for y in marginal(L)]


def r256(n):
    return (n + 255) // 256 * 256


def test_size_relations_and_ignored_bits(L):
    n = 0
    for shape, B, chunk, flags in size_grid(L):
        _, Lz, K, _ = shape
        ymarg = flags & (L.OBJ_MARGINAL_Y | L.OBJ_MARGINAL_Y_IW)
        d, plain = dims(L, shape, B, chunk, flags), dims(L, shape, B, chunk)
        # y summed out: the marginal bits are ignored like the maskable ones, and gmvae_posterior_y's workspace is
        # gmvae_iw_bound_enum_y's plus the state [B][K][3] fp64
        rc, enum = query(L, "iw_bound_enum_y", d, L.MODEL_GMVAE)
        assert rc == 0 and (rc, enum) == query(L, "iw_bound_enum_y", plain, L.MODEL_GMVAE), (shape, B, chunk, flags)
        assert query(L, "posterior_y", d, L.MODEL_GMVAE) == (0, enum + r256(B * K * 24)), (shape, B, chunk, flags)
        for model in (L.MODEL_VAE, L.MODEL_VAE_GMP, L.MODEL_GMVAE):
            got = query(L, "iw_bound", d, model)
            if ymarg:         # gmvae_iw_bound refuses both bits; check_dims knows them for the GMVAE alone
                assert got[0] == (E_DIMS if model == L.MODEL_GMVAE else E_MODEL), (shape, B, chunk, flags, model)
            else:
                assert got[0] == 0 and got == query(L, "iw_bound", plain, model), (shape, B, chunk, flags, model)
        # gmvae_posterior_component's workspace is gmvae_iw_bound's plus the state [B][K][2] fp64, ess [B][3] fp64, the chunk's
        # [B S][max(K, L)] side buffer and gmp_consts' inv [K][L] and cst [K]
        rc, pc = query(L, "posterior_component", d, L.MODEL_VAE_GMP)
        if ymarg:
            assert rc == E_MODEL, (shape, B, chunk, flags)
        else:
            own = (B * K * 16, B * 24, B * chunk * max(K, Lz) * 4, K * Lz * 4, K * 4)
            assert rc == 0 and pc == query(L, "iw_bound", d, L.MODEL_VAE_GMP)[1] + sum(map(r256, own)), (shape, B, chunk, flags)
        n += 1
    assert n == len(SHAPES) * len(BATCHES) * 16 * 4


def test_queries_refuse_what_the_entry_points_refuse(L):
    d = dims(L, SHAPES[1], 8, 5)
    for kind in KINDS:
        assert query(L, kind, dims(L, SHAPES[1], 0, 5), L.MODEL_GMVAE)[0] == E_DIMS
        assert getattr(L.lib, f"gmvae_{kind}_workspace_bytes")(None, L.MODEL_GMVAE, C.byref(C.c_uint64())) == E_NULL
    for model in (L.MODEL_VAE, L.MODEL_VAE_GMP):
        assert query(L, "iw_bound_enum_y", d, model)[0] == E_MODEL and query(L, "posterior_y", d, model)[0] == E_MODEL
    for model in (L.MODEL_VAE, L.MODEL_GMVAE):
        assert query(L, "posterior_component", d, model)[0] == E_MODEL
    assert query(L, "iw_bound", d, 3)[0] == E_MODEL
    for kind, model in zip(KINDS, (L.MODEL_VAE, L.MODEL_GMVAE, L.MODEL_GMVAE, L.MODEL_VAE_GMP)):
        assert getattr(L.lib, f"gmvae_{kind}_workspace_bytes")(C.byref(d), model, None) == E_NULL


P = 1 << 20            # a fake device pointer, never dereferenced: every case below fails a check before any launch


def call(L, kind, d, model, n=10, x=P, params=P, out=(None, None, None), tail=P, ws=P):
    """gmvae_<kind> on fake pointers and the NULL stream; d None: NULL dims."""
    outs = [None if o is None else C.c_void_p(o) for o in (out[:2] if kind.startswith("iw_bound") else out)]
    ptr = lambda a: None if a is None else C.c_void_p(a)
    return getattr(L.lib, f"gmvae_{kind}")(None if d is None else C.byref(d), model, ptr(x), ptr(params), n, *outs, ptr(tail),
                                           ptr(ws), 0, 0, None)


def failing_cases(L):
    """(kind, what, keyword arguments of call(), the documented code): every case fails at least one check."""
    shape, K = SHAPES[1], SHAPES[1][2]
    own = dict(zip(KINDS, (L.MODEL_GMVAE, L.MODEL_GMVAE, L.MODEL_GMVAE, L.MODEL_VAE_GMP)))
    cases = []
    for kind in KINDS:
        per = K if kind in ENUM_Y else 1                       # Philox rows per sample
        n_outs = 2 if kind.startswith("iw_bound") else 3
        for m in (0, max(maskable(L))):                        # the same answers with every maskable bit set
            d, model = dims(L, shape, 8, 5, m), own[kind]
            add = lambda what, code, **kw: cases.append((kind, f"{what} flags={m}", dict(dict(d=d, model=model), **kw), code))
            # --- dims
            add("NULL dims", E_NULL, d=None)
            add("unknown model", E_MODEL, model=3)
            add("B = 0", E_DIMS, d=dims(L, shape, 0, 5, m))
            add("chunk = 0", E_DIMS, d=dims(L, shape, 8, 0, m))
            add("B S > 2^30", E_DIMS, d=dims(L, shape, 1 << 20, 1 << 11, m))
            if kind in ENUM_Y:
                add("B S K > 2^30", E_DIMS, d=dims(L, shape, 1 << 20, 1 << 8, m))             # (B S = 2^28 passes)
                add("VAE", E_MODEL, model=L.MODEL_VAE)
                add("VAE_GMP", E_MODEL, model=L.MODEL_VAE_GMP)
            else:
                for y in marginal(L)[1:]:                      # the Gumbel bound and the VAE_GMP's posterior refuse the bits
                    add(f"marginal bits {y}", E_DIMS if model == L.MODEL_GMVAE else E_MODEL, d=dims(L, shape, 8, 1, m | y))
            if kind == "posterior_component":
                add("VAE", E_MODEL, model=L.MODEL_VAE)
                add("GMVAE", E_MODEL, model=L.MODEL_GMVAE)
            # --- NULL, after the dims and before the range and the alignment
            for name in ("x", "params", "tail", "ws"):
                add(f"NULL {name}", E_NULL, **{name: None})
            add("bad dims before NULL x", E_DIMS, d=dims(L, shape, 0, 5, m), x=None)
            add("NULL x before n = 0", E_NULL, x=None, n=0)
            add("NULL workspace before an unaligned x", E_NULL, ws=None, x=P + 4)
            # --- the range of n_samples: n > 0 and (row0 + B) n [K] < 2^38, Philox's row field
            add("n = 0", E_DIMS, n=0)
            add("n = 0 before an unaligned x", E_DIMS, n=0, x=P + 4)
            row0 = (1 << 38) // (1000 * per) - 7                # (row0 + 8) 1000 [K] > 2^38 - 1 >= (row0 + 7) 1000 [K]
            add("(row0 + B) n [K] >= 2^38", E_DIMS, d=dims(L, shape, 8, 5, m, row0=row0), n=1000)
            add("row0 + B wraps", E_DIMS, d=dims(L, shape, 8, 5, m, row0=(1 << 64) - 4))
            # --- alignment: x, params, tail, the workspace and every output given
            for name in ("x", "params", "tail", "ws"):
                add(f"unaligned {name}", E_ALIGN, **{name: P + 4})
            for i in range(n_outs):
                add(f"unaligned output {i}", E_ALIGN, out=tuple(P + 8 if j == i else None for j in range(3)))
                add(f"unaligned output {i}, the others given", E_ALIGN, out=tuple(P + 8 if j == i else P for j in range(3)))
    return cases


def test_every_failing_argument_returns_its_documented_code(L):
    cases = failing_cases(L)
    assert len(cases) > 200
    for kind, what, kw, code in cases:
        assert call(L, kind, **kw) == code, (kind, what)


def test_the_philox_row_limit_is_exact(L):
    # the largest row0 each kind still takes at B = 8, n = 1000 fails only LATER checks (here: the unaligned x), one more row fails
    # the range check
    shape, K = SHAPES[1], SHAPES[1][2]
    for kind, model in zip(KINDS, (L.MODEL_GMVAE, L.MODEL_GMVAE, L.MODEL_GMVAE, L.MODEL_VAE_GMP)):
        per = K if kind in ENUM_Y else 1
        last = ((1 << 38) - 1) // (1000 * per) - 8
        assert call(L, kind, dims(L, shape, 8, 5, row0=last), model, n=1000, x=P + 4) == E_ALIGN, kind
        assert call(L, kind, dims(L, shape, 8, 5, row0=last + 1), model, n=1000, x=P + 4) == E_DIMS, kind
