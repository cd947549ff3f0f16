"""A guarded arena for device buffers -- test infrastructure, a plain module; works on any torch device, "cpu" included.

One torch.uint8 tensor backs the arena, every byte 0xFF at first: a NaN read as fp32 or fp64, 255 read as a {0,1} byte.
place() hands out typed views of it: each starts at a multiple of 256 bytes from the arena's (256-byte aligned) base, is exactly
as long as asked, and has a guard band of max(64 KiB, 128 * row_pitch_bytes) in front of it and behind it (128 rows: the tallest
tile any kernel of the library stores -- the large GEMM configuration and the plane tiles -- so the band is a floor for an overrun
of one tile, not a claim about larger ones).  snapshot() clones the used part on the device just before a call; check(), after the
call, compares the two on the device and fails if a byte differs anywhere but inside the ranges marked writable: the guard bands,
and every buffer (or part of one) the call may only read.  A stray store therefore lands in memory the test owns and is reported
by the buffer's name, the side, the distance from the buffer's edge, and the byte before and after; nothing here is meant to fault.

Plain is the same interface over separate exact-size tensors without guards: the reference run of a bit-identity comparison."""
import torch

ALIGN = 256
MIN_BAND = 64 * 1024
TILE_ROWS = 128
FILL = 0xFF


def band_bytes(row_pitch_bytes):
    return max(MIN_BAND, TILE_ROWS * int(row_pitch_bytes))


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


class GuardHit(AssertionError):
    """check() found bytes changed outside the writable ranges.  hits: one dict per region that changed -- name, side ("front" /
    "behind" of the buffer, or "inside" it), distance (bytes from the buffer's edge to the nearest changed byte: 1 is the byte next
    to the buffer; inside, the byte's offset from the buffer's start), farthest (the same for the farthest changed byte), count,
    old and new (the nearest byte before and after)."""

    def __init__(self, hits):
        self.hits = hits
        lines = [f"{h['name']}: {h['count']} byte(s) changed {h['side']}"
                 + (f" the buffer, nearest {h['distance']} and farthest {h['farthest']} byte(s) from its edge" if h["side"] != "inside"
                    else f" a range the call may only read, first at offset {h['distance']}, last at {h['farthest']}")
                 + f"; nearest byte 0x{h['old']:02X} -> 0x{h['new']:02X}" for h in hits]
        super().__init__("bytes changed outside the call's writable set:\n  " + "\n  ".join(lines))


class _Buf:
    def __init__(self, name, start, nbytes, band, writable):
        self.name, self.start, self.nbytes, self.band = name, start, nbytes, band
        self.writable = writable

    @property
    def end(self):
        return self.start + self.nbytes


def _ranges(writable, nbytes):
    """writable as byte ranges of the buffer: True -> all of it, False / None -> none, else an iterable of (lo, hi)."""
    if writable is True:
        return [(0, nbytes)]
    if not writable:
        return []
    out = []
    for lo, hi in writable:
        lo, hi = int(lo), int(hi)
        assert 0 <= lo <= hi <= nbytes, (lo, hi, nbytes)
        out.append((lo, hi))
    return out


class Arena:
    def __init__(self, device, capacity):
        """capacity: bytes of backing store (place() fails loudly when it runs out); only the used part is ever cloned or compared."""
        self.device = torch.device(device)
        raw = torch.full((int(capacity) + ALIGN,), FILL, dtype=torch.uint8, device=self.device)
        skew = (-raw.data_ptr()) % ALIGN
        self.mem = raw[skew:skew + int(capacity)]
        self.capacity = int(capacity)
        self.bufs = []
        self.used = 0
        self.peak = 0
        self.snap = None

    def reset(self):
        """Forget every placement; the used part goes back to 0xFF."""
        self.mem[:self.used].fill_(FILL)
        self.bufs, self.used, self.snap = [], 0, None

    def place(self, name, nbytes, row_pitch_bytes, writable, dtype=torch.uint8):
        """A view of `dtype` over exactly `nbytes` bytes (a multiple of the element size), 0xFF everywhere.  writable: True, False, or
        byte ranges [(lo, hi), ...] of the buffer that the next call may change (set_writable changes it between calls)."""
        nbytes = int(nbytes)
        item = torch.empty((), dtype=dtype).element_size()
        assert nbytes >= 0 and nbytes % item == 0, (name, nbytes, dtype)
        assert all(b.name != name for b in self.bufs), f"{name} is placed twice"
        band = band_bytes(row_pitch_bytes)
        start = _up(self.used + band)
        if start + nbytes + band > self.capacity:
            raise MemoryError(f"arena of {self.capacity} bytes is full: {name} needs [{start}, {start + nbytes + band})")
        b = _Buf(name, start, nbytes, band, _ranges(writable, nbytes))
        self.bufs.append(b)
        self.used = b.end + band
        self.peak = max(self.peak, self.used)
        self.snap = None
        return self.mem[b.start:b.end].view(dtype)

    def buf(self, name):
        for b in self.bufs:
            if b.name == name:
                return b
        raise KeyError(name)

    def view(self, name, dtype=torch.uint8):
        b = self.buf(name)
        return self.mem[b.start:b.end].view(dtype)

    def set_writable(self, name, writable):
        b = self.buf(name)
        b.writable = _ranges(writable, b.nbytes)

    def snapshot(self):
        """Clone the used part on the device: call it just before the call under test, after every input is in place."""
        self._sync()
        self.snap = self.mem[:self.used].clone()

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check(self):
        """After the call (synchronises first): every byte outside the writable ranges equals the snapshot, or GuardHit."""
        assert self.snap is not None and self.snap.numel() == self.used, "snapshot() comes before the call, after the last place()"
        self._sync()
        diff = self.mem[:self.used] != self.snap
        for b in self.bufs:
            for lo, hi in b.writable:
                diff[b.start + lo:b.start + hi] = False
        if not bool(diff.any()):
            return
        hits = []
        for i, b in enumerate(self.bufs):
            # the space between two buffers is split where the earlier one's band ends: the alignment padding goes to the later one
            front_lo = self.bufs[i - 1].end + self.bufs[i - 1].band if i else 0
            for side, lo, hi in (("front", front_lo, b.start), ("inside", b.start, b.end), ("behind", b.end, b.end + b.band)):
                at = diff[lo:hi].nonzero().flatten()
                if at.numel() == 0:
                    continue
                first, last = lo + int(at[0]), lo + int(at[-1])
                near = last if side == "front" else first
                far = first if side == "front" else last
                dist = {"front": lambda o: b.start - o, "inside": lambda o: o - b.start, "behind": lambda o: o - b.end + 1}[side]
                hits.append({"name": b.name, "side": side, "distance": dist(near), "farthest": dist(far), "count": int(at.numel()),
                             "old": int(self.snap[near]), "new": int(self.mem[near])})
        raise GuardHit(hits)


class Plain:
    """Arena's interface over separate exact-size tensors, no guards: what a caller without an arena allocates."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs = {}

    def reset(self):
        self.bufs = {}

    def place(self, name, nbytes, row_pitch_bytes, writable, dtype=torch.uint8):
        assert name not in self.bufs, f"{name} is placed twice"
        t = torch.full((int(nbytes),), FILL, dtype=torch.uint8, device=self.device)
        self.bufs[name] = t
        return t.view(dtype)

    def view(self, name, dtype=torch.uint8):
        return self.bufs[name].view(dtype)

    def set_writable(self, name, writable):
        pass

    def snapshot(self):
        pass

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
