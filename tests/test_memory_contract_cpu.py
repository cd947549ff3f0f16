"""tests/arena.py on the CPU: the guarded arena reports what it must and nothing else.  The device tests of
tests/test_memory_contract.py lean on exactly these properties."""
import pytest
import torch

import arena as A

# (name, bytes, row pitch in bytes, writable, dtype): odd lengths, a pitch past 64 KiB / 128, a partly writable buffer
SPEC = [("x", 9 * 97, 97, False, torch.uint8),
        ("params", 4 * 1028, 4 * 24, False, torch.float32),
        ("grads", 4 * (1028 + 8), 4 * 24, True, torch.float32),
        ("wide", 4 * 3 * 3072, 4 * 3072, True, torch.float32),
        ("step_dev", 32, 16, [(0, 16)], torch.int64),
        ("tail", 32, 32, True, torch.float32),
        ("f64", 8 * 5, 8, False, torch.float64),
        ("empty_rows", 0, 4, True, torch.float32)]


def _arena():
    ar = A.Arena("cpu", 4 << 20)
    views = {name: ar.place(name, n, pitch, w, dtype=dt) for name, n, pitch, w, dt in SPEC}
    return ar, views


def test_views_are_aligned_exact_and_poisoned():
    ar, views = _arena()
    prev_end = prev_band = 0
    for name, n, pitch, w, dt in SPEC:
        v, b = views[name], ar.buf(name)
        assert v.dtype == dt and v.numel() * v.element_size() == n == b.nbytes
        assert b.start % 256 == 0 and ar.mem.data_ptr() % 256 == 0
        assert n == 0 or v.data_ptr() - ar.mem.data_ptr() == b.start        # (torch gives an empty view no address)
        band = max(64 * 1024, 128 * pitch)
        assert b.band == band == A.band_bytes(pitch)
        assert b.start - prev_end >= band + prev_band                       # this one's front band behind the previous one's own
        prev_end, prev_band = b.end, band
        if dt.is_floating_point:
            assert torch.isnan(v).all()
        elif dt == torch.uint8:
            assert (v == 255).all()
    assert ar.used == prev_end + ar.buf(SPEC[-1][0]).band <= ar.capacity
    assert (ar.mem[:ar.used] == 0xFF).all()
    assert A.band_bytes(4 * 3072) == 128 * 4 * 3072 > A.MIN_BAND


def test_arena_refuses_what_it_cannot_hold():
    ar = A.Arena("cpu", 3 * 64 * 1024)
    ar.place("a", 100, 4, True)
    with pytest.raises(MemoryError):
        ar.place("b", 64 * 1024, 4, True)
    with pytest.raises(AssertionError):
        ar.place("a", 4, 4, True)
    with pytest.raises(AssertionError):
        ar.place("c", 6, 4, True, dtype=torch.float32)


def test_writes_inside_writable_ranges_pass():
    ar, views = _arena()
    ar.snapshot()
    views["grads"].fill_(1.5)
    views["wide"].zero_()
    views["tail"][:] = 3.0
    views["step_dev"][:2] = 7                       # the two writable words
    ar.check()
    ar.check()                                      # (checking changes nothing)


def _plant(ar, offset):
    old = int(ar.mem[offset])
    ar.mem[offset] = old ^ 0x5A
    return old, old ^ 0x5A


@pytest.mark.parametrize("name", [s[0] for s in SPEC])
@pytest.mark.parametrize("side,where", [("front", "near"), ("front", "far"), ("behind", "near"), ("behind", "far")])
def test_one_byte_in_a_guard_band_is_reported(name, side, where):
    """The first and the last byte of each band, for every buffer, writable or not."""
    ar, _ = _arena()
    b = ar.buf(name)
    dist = 1 if where == "near" else b.band
    off = b.start - dist if side == "front" else b.end + dist - 1
    ar.snapshot()
    old, new = _plant(ar, off)
    with pytest.raises(A.GuardHit) as e:
        ar.check()
    assert len(e.value.hits) == 1
    h = e.value.hits[0]
    assert (h["name"], h["side"], h["distance"], h["farthest"], h["count"], h["old"], h["new"]) == (name, side, dist, dist, 1, old, new)
    assert name in str(e.value) and side in str(e.value) and f"0x{old:02X} -> 0x{new:02X}" in str(e.value)
    ar.mem[off] = old
    ar.check()


@pytest.mark.parametrize("name,offset", [("x", 0), ("x", 9 * 97 - 1), ("params", 4 * 1028 - 1), ("f64", 17),
                                         ("step_dev", 16), ("step_dev", 31)])
def test_one_byte_inside_a_read_only_range_is_reported(name, offset):
    ar, views = _arena()
    ar.snapshot()
    old, new = _plant(ar, ar.buf(name).start + offset)
    views["step_dev"][0] = 1                        # a legal write next to it stays unreported
    with pytest.raises(A.GuardHit) as e:
        ar.check()
    h, = e.value.hits
    assert (h["name"], h["side"], h["distance"], h["count"], h["old"], h["new"]) == (name, "inside", offset, 1, old, new)


def test_an_overrun_is_attributed_to_the_buffer_it_left():
    """A ragged tile's worth of stores past `grads` and a few before `tail`: two hits, nearest and farthest byte of each."""
    ar, views = _arena()
    g, t = ar.buf("grads"), ar.buf("tail")
    ar.snapshot()
    ar.mem[g.end:g.end + 16 * 4].zero_()
    ar.mem[t.start - 8:t.start - 4].zero_()
    with pytest.raises(A.GuardHit) as e:
        ar.check()
    got = [(h["name"], h["side"], h["distance"], h["farthest"], h["count"]) for h in e.value.hits]
    assert got == [("grads", "behind", 1, 64, 64), ("tail", "front", 5, 8, 4)]


def test_set_writable_and_reset():
    ar, views = _arena()
    ar.set_writable("x", True)
    ar.set_writable("grads", [(0, 16)])
    ar.snapshot()
    views["x"].zero_()
    views["grads"][:4] = 0.0
    ar.check()
    views["grads"][4] = 0.0
    with pytest.raises(A.GuardHit) as e:
        ar.check()
    assert [(h["name"], h["side"], h["distance"]) for h in e.value.hits] == [("grads", "inside", 16)]
    used = ar.used
    ar.reset()
    assert ar.used == 0 and ar.bufs == [] and (ar.mem[:used] == 0xFF).all() and ar.peak == used
    with pytest.raises(AssertionError):
        ar.check()                                  # no snapshot


def test_plain_has_the_same_interface():
    pl = A.Plain("cpu")
    v = pl.place("z", 40, 8, False, dtype=torch.float64)
    assert v.numel() == 5 and torch.isnan(v).all() and pl.view("z").numel() == 40
    pl.snapshot()
    pl.set_writable("z", True)
    pl.check()
