"""A guarded arena: ONE uint8 allocation per test out of which the test carves every buffer it hands to the library.

Why: torch's caching allocator rounds every block up and aligns it to 512 bytes, so an exact-size torch tensor hides a
write past its end, and an address that is only as aligned as the header promises is never seen.  Here every region is
exactly as long as asked, sits at exactly the residue mod 16 that was asked for (and is NOT better aligned than that), and
has a guard band on both sides that starts at the very next byte.  Guards and regions are filled from a seeded byte
pattern (a function of seed and arena offset, not a constant: a kernel that writes a constant back cannot pass), and
check() / unchanged() compare them with that pattern on the device the arena lives on.

Safety rule (part of the design, enforced by carve()): every address given to the library lies inside this one live
allocation, with guards of at least `min_guard` bytes (1 MiB on a GPU) on each side of every region; callers size guards
with guard_bytes(frame_bytes): at least 1 MiB and at least one frame, capped at 16 MiB.  A plausible overrun (a vector, a
row, a tile, a frame) then lands in memory the process owns and shows up as a failed check(), never as a device fault.

The layout arithmetic (place) is pure integer code and the whole class works on CPU tensors, so tests/test_arena_cpu.py
pins it without a GPU."""
import numpy as np
import torch

MIN_GUARD = 1 << 20
MAX_GUARD = 16 << 20


class ArenaError(AssertionError):
    """A guard or a read-only region no longer holds its pattern."""

    def __init__(self, region, side, offset, count, what):
        super().__init__(f"arena: {what} '{region}' ({side}): {count} byte(s) changed, first at offset {offset}")
        self.region, self.side, self.offset, self.count = region, side, offset, count


def guard_bytes(frame_bytes):
    """The guard the safety rule asks for around buffers whose natural overrun unit is `frame_bytes`."""
    return int(min(max(MIN_GUARD, int(frame_bytes)), MAX_GUARD))


def place(cursor, nbytes, offset_mod16=0, guard=MIN_GUARD, align=16):
    """Where a region of `nbytes` goes when every address below `cursor` is taken: -> (start, end, next_cursor), absolute
    addresses.  start is the lowest address >= cursor + guard with start % align == offset_mod16 that is not better
    aligned than asked: for a residue of 0, start % (2 * align) == align (a non-zero residue fixes the alignment by its
    lowest set bit).  [cursor, start) is the guard before (>= guard bytes), [end, next_cursor) the guard after (exactly
    guard bytes, beginning at the byte after the region)."""
    if align < 16 or align & (align - 1):
        raise ValueError("align must be a power of two >= 16")
    if not 0 <= offset_mod16 < align:
        raise ValueError("offset_mod16 must be in [0, align)")
    if nbytes < 0 or guard < 1:
        raise ValueError("nbytes >= 0 and guard >= 1")
    period, want = (2 * align, align) if offset_mod16 == 0 else (align, offset_mod16)
    lo = cursor + guard
    start = lo + ((want - lo) % period)
    return start, start + nbytes, start + nbytes + guard


def capacity_for(specs):
    """An arena size that holds regions [(nbytes, guard[, align])...] whatever the base address is."""
    return sum(s[0] + 2 * s[1] + 2 * (s[2] if len(s) > 2 else 16) for s in specs) + 64


def pattern(n, seed, offset, device="cpu"):
    """n seeded bytes: a 32-bit integer hash of (seed, offset + i), lowest byte.  Chunked: 8 temporaries of int64."""
    out = torch.empty(n, dtype=torch.uint8, device=device)
    M = 0xFFFFFFFF
    step = 1 << 22
    for a in range(0, n, step):
        b = min(n, a + step)
        v = torch.arange(offset + a, offset + b, dtype=torch.int64, device=device)
        v = (v + (int(seed) + 1) * 0x9E3779B1) & M
        v = (v ^ (v >> 16)) * 0x85EBCA6B & M
        v = (v ^ (v >> 13)) * 0xC2B2AE35 & M
        v = v ^ (v >> 16)
        out[a:b] = (v & 0xFF).to(torch.uint8)
    return out


def _fill_spec(fill):
    if fill in ("zeros", "ones"):
        return fill, 0
    if isinstance(fill, tuple) and len(fill) == 2 and fill[0] == "noise":
        return "noise", int(fill[1])
    raise ValueError(f"fill must be 'zeros', 'ones' or noise(seed), not {fill!r}")


def noise(seed):
    return ("noise", int(seed))


class Arena:
    def __init__(self, capacity, device="cpu", seed=0, min_guard=None):
        self.device = torch.device(device)
        self.min_guard = (MIN_GUARD if self.device.type == "cuda" else 1) if min_guard is None else int(min_guard)
        self.buf = torch.empty(int(capacity), dtype=torch.uint8, device=self.device)
        self.base = self.buf.data_ptr()
        self.cursor = 0            # arena offset of the first byte not yet given out
        self.seed = int(seed)
        self.regions = {}          # name -> dict(start, end, g0, g1): arena offsets; guards [g0, start) and [end, g1)
        self.expected = {}         # name -> ("fill", kind, seed) | ("data", clone): what unchanged() compares with

    # ---- layout
    def carve(self, name, nbytes, offset_mod16=0, guard=MIN_GUARD, align=16):
        """-> uint8 view of exactly nbytes bytes at an address = offset_mod16 (mod align), no better aligned; guards of
        `guard` bytes on both sides, filled from the arena's seed.  The region itself starts as noise too."""
        if name in self.regions:
            raise ValueError(f"region {name!r} exists")
        if guard < self.min_guard:
            raise ValueError(f"guard of {guard} bytes is below the arena's minimum of {self.min_guard}")
        start, end, nxt = place(self.base + self.cursor, int(nbytes), offset_mod16, int(guard), align)
        start, end, nxt = start - self.base, end - self.base, nxt - self.base
        if nxt > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is full ({name!r} ends at {nxt})")
        self.regions[name] = dict(start=start, end=end, g0=self.cursor, g1=nxt)
        self.cursor = nxt
        self._fill_guards(name)
        self.fill(name, noise(self.seed ^ 0x5a5a))
        return self.view(name)

    def view(self, name):
        r = self.regions[name]
        return self.buf[r["start"]:r["end"]]

    def ptr(self, name):
        return self.base + self.regions[name]["start"]

    # ---- contents
    def _fill_guards(self, name):
        r = self.regions[name]
        self.buf[r["g0"]:r["start"]] = pattern(r["start"] - r["g0"], self.seed, r["g0"], self.device)
        self.buf[r["end"]:r["g1"]] = pattern(r["g1"] - r["end"], self.seed, r["end"], self.device)

    def reseed(self, seed):
        """New guard pattern everywhere (regions keep their contents)."""
        self.seed = int(seed)
        for name in self.regions:
            self._fill_guards(name)

    def fill(self, name, fill):
        kind, seed = _fill_spec(fill)
        r = self.regions[name]
        v = self.buf[r["start"]:r["end"]]
        if kind == "zeros":
            v.zero_()
        elif kind == "ones":
            v.fill_(0xFF)
        else:
            v.copy_(pattern(v.numel(), seed, r["start"], self.device))
        self.expected[name] = ("fill", kind, seed)

    def put(self, name, data):
        """Copy a numpy array / tensor (any dtype, exactly the region's size in bytes) into the region."""
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        v = self.view(name)
        if raw.size != v.numel():
            raise ValueError(f"{name!r} holds {v.numel()} bytes, data has {raw.size}")
        t = torch.from_numpy(raw.copy()).to(self.device)
        v.copy_(t)
        self.expected[name] = ("data", t)

    def get(self, name, dtype=np.uint8):
        return self.view(name).cpu().numpy().view(dtype)

    def _expected(self, name):
        e = self.expected[name]
        if e[0] == "data":
            return e[1]
        r = self.regions[name]
        n = r["end"] - r["start"]
        if e[1] == "zeros":
            return torch.zeros(n, dtype=torch.uint8, device=self.device)
        if e[1] == "ones":
            return torch.full((n,), 0xFF, dtype=torch.uint8, device=self.device)
        return pattern(n, e[2], r["start"], self.device)

    # ---- checks
    @staticmethod
    def _diff(got, want):
        bad = got != want
        count = int(bad.sum().item())
        if not count:
            return None
        return int(torch.nonzero(bad)[0].item()), count

    def check(self):
        """Every guard still holds its pattern, or ArenaError with the region, the side, the offset of the first changed
        byte (after: 0 is the byte right behind the region; before: negative, -1 is the byte right in front of it) and the
        number of changed bytes."""
        for name, r in self.regions.items():
            d = self._diff(self.buf[r["end"]:r["g1"]], pattern(r["g1"] - r["end"], self.seed, r["end"], self.device))
            if d:
                raise ArenaError(name, "after", d[0], d[1], "guard of")
            d = self._diff(self.buf[r["g0"]:r["start"]], pattern(r["start"] - r["g0"], self.seed, r["g0"], self.device))
            if d:
                raise ArenaError(name, "before", d[0] - (r["start"] - r["g0"]), d[1], "guard of")

    def unchanged(self, name):
        """The region still holds what fill() / put() left in it (inputs, tables, gates, an output after a refused call)."""
        d = self._diff(self.view(name), self._expected(name))
        if d:
            raise ArenaError(name, "inside", d[0], d[1], "read-only region")
