"""Inputs and the model of the find tests (tests/test_find.py, tests/test_cli_find.py).

The model of everything is hits(D, pat): every p with D[p:p + m] == pat, found by bytes.find in a loop that advances by 1.
borders(align, length, m) restates where the work of the find kernels (bzx_find.hip) changes hands inside a run of
`length` bytes that starts `align` bytes behind a 16-byte boundary: head to body, one lane's 16 bytes to the next, one
64-lane step to the next, one wave's section to the next, one workgroup's tile to the next, body to tail, and the last
start position that has m bytes in front of it."""
import random

import numpy as np

LANE_BYTES = 16                  # one load
STEP_BYTES = 64 * LANE_BYTES     # one load per lane of a wave
WAVES = 4                        # sections of a tile
PALETTE = bytes([0x00, 0x7F, 0x80, 0xFF, 0x41, 0x0A])
M_LIST = (1, 2, 3, 4, 5, 15, 16, 17, 255, 256)


def hits(data, pat):
    """The model: all start positions, ascending, overlapping ones included."""
    data, pat = bytes(data), bytes(pat)
    out = []
    i = data.find(pat)
    while i >= 0:
        out.append(i)
        i = data.find(pat, i + 1)
    return out


def borders(align, length, m, tile_bytes):
    """Sorted positions b in [0, length] where the byte b - 1 and the byte b belong to different hands."""
    head = min(length, (16 - align) & 15)
    body_end = max(head, length - (align + length) % 16)
    out = {head, body_end, max(length - m, 0)}
    lanes = list(range(head, length + 1, LANE_BYTES))
    out.update(lanes if len(lanes) <= 140 else lanes[:3] + lanes[-3:])
    for unit in (STEP_BYTES, tile_bytes // WAVES, tile_bytes):
        for b in range((-align) % unit, length + 1, unit):
            out.add(b)
    return sorted(b for b in out if 0 <= b <= length)


def pattern(m, seed):
    """m seeded bytes of the palette (0x00, 0x7F, 0x80 and 0xFF among them)."""
    rnd = random.Random(1000 * m + seed)
    return bytes(rnd.choice(PALETTE) for _ in range(m))


def filler(n, seed):
    return bytearray(np.frombuffer(PALETTE, dtype=np.uint8)[np.random.default_rng(seed).integers(0, len(PALETTE), n)].tobytes())


def near_misses(pat):
    """The pattern with another first byte, with another last byte, and with bit 7 of one byte flipped."""
    a, b, c = bytearray(pat), bytearray(pat), bytearray(pat)
    a[0] ^= 0x01
    b[-1] ^= 0x01
    c[len(pat) // 2] ^= 0x80
    return bytes(a), bytes(b), bytes(c)


def wanted_starts(align, length, m, tile_bytes):
    """Starts that put a pattern's first byte on b - 1, b, b + 1 of every border b, its last byte there, and its middle
    across b; one that ends exactly at the run's end; and the two that miss the run by one byte, in front and behind."""
    w = {length - m, length - m + 1, -1, 0}
    for b in borders(align, length, m, tile_bytes):
        for d in (-1, 0, 1):
            w.update((b + d, b + d - m + 1))
        w.add(b - m // 2)
    return sorted(s for s in w if -1 <= s <= length - m + 1)


def groups(starts, m, max_groups=None):
    """The starts in as few lists as it takes for no two patterns of a list to overlap (greedy, ascending)."""
    out = []
    for s in starts:
        for g in out:
            if g[-1] + m <= s:
                g.append(s)
                break
        else:
            if max_groups is None or len(out) < max_groups:
                out.append([s])
    return out


class Layout:
    """A buffer for one bzx_stage_find call: segments appended at chosen alignments, each with at least two bytes of
    other content on both sides."""

    def __init__(self, seed):
        self.buf = bytearray(filler(32, seed))
        self.segs = []
        self.seed = seed

    def add(self, align, length):
        """-> the segment's offset; its bytes are filler so far."""
        off = len(self.buf) + 2
        off += (align - off) % 16
        self.buf += filler(off + length + 2 - len(self.buf), self.seed + len(self.segs) + 1)
        self.segs.append((off, length))
        return off

    def plant(self, off, length, s, what):
        """`what` at position s of the segment at off, clipped to one byte in front of and one behind the segment."""
        a, z = max(s, -1), min(s + len(what), length + 1)
        if a < z:
            self.buf[off + a:off + z] = what[a - s:z - s]

    def fill(self, off, length, what):
        self.buf[off:off + length] = (bytes(what) * (length // len(what) + 1))[:length]

    def model(self, pat):
        """-> ([count per segment], [the hits of all segments in segment order, relative to their segment])"""
        per = [hits(self.buf[o:o + ln], pat) for o, ln in self.segs]
        return [len(h) for h in per], [p for h in per for p in h]


def lengths(m, tile_bytes, big=True):
    ls = {0, 1, m - 1, m, m + 1, 15, 16, 17, 1023, 1024, 1025}
    if big:
        ls |= {tile_bytes - 1, tile_bytes, tile_bytes + 1, 2 * tile_bytes + 17}
    return sorted(ls)


def planted_layout(m, shapes, tile_bytes, seed, max_groups=None):
    """One layout with, for every (align, length) of shapes, as many copies of the segment as it takes to plant the
    pattern at every wanted start, and one copy filled with near misses around single patterns.
    -> (layout, pattern, [(segment number, start)] of the patterns planted wholly inside a segment)"""
    pat = pattern(m, seed)
    lay = Layout(seed)
    inside = []
    for align, length in shapes:
        want = wanted_starts(align, length, m, tile_bytes)
        gs = groups(want, m, max_groups)
        if max_groups is None:
            assert sorted(s for g in gs for s in g) == want
        for g in gs or [[]]:
            off = lay.add(align, length)
            for s in g:
                lay.plant(off, length, s, pat)
                if 0 <= s <= length - m:
                    inside.append((len(lay.segs) - 1, s))
        off = lay.add(align, length)
        lay.fill(off, length, b"".join(near_misses(pat)) + pat)
    return lay, pat, inside


# ---- end to end --------------------------------------------------------------------------------------------------------------
def plant_around(data, pat, plan):
    """plan: [(c, spread)].  pat planted so that it starts on c + d and ends on c + d - 1 for every d of the spread, and
    lies across c, wherever that does not overlap an earlier planting (so the first d of a spread is served first)."""
    d = bytearray(data)
    m = len(pat)
    taken = []
    for c, spread in plan:
        for s in [c + x for x in spread] + [c + x - m for x in spread] + [c - m // 2, c - 1 - m // 3]:
            if s < 0 or s + m > len(d) or any(a < s + m and s < z for a, z in taken):
                continue
            d[s:s + m] = pat
            taken.append((s, s + m))
    return bytes(d)
