"""Inputs and models of the record tests (tests/test_records.py, tests/test_cli_records.py).

The model of everything is np.flatnonzero(a == delim): rec_start, the record table, the planners.
borders(align, length) restates where the work of the two record kernels (bzx_records.hip: rec_cut, rec_sections, the
select kernel's walk) changes hands inside a segment of `length` bytes that starts `align` bytes behind a 16-byte
boundary: head to body, one lane's 16 bytes to the next, one tile of 64 lanes to the next, one wave's share to the next,
body to tail."""
import random

import numpy as np

REC_NT = 512                     # lanes of a workgroup of either kernel
REC_NW = REC_NT // 64            # waves: each takes a contiguous share of whole tiles
LANE_BYTES = 16                  # one load
TILE_BYTES = 64 * LANE_BYTES     # one load per lane of a wave
DELIMS = (0x00, 0x0A, 0x7F, 0x80, 0xFF)
MiB = 1 << 20


def cut(align, length):
    """-> (head bytes, 16-byte loads of the body, tail bytes, loads of a wave's share)."""
    head = min(length, (16 - align) & 15)
    nvec = (length - head) // 16
    tail = length - head - nvec * 16
    ntile = (nvec + 63) // 64
    share = (ntile + REC_NW - 1) // REC_NW * 64
    return head, nvec, tail, share


def borders(align, length):
    """Sorted positions b in [0, length] where the byte b - 1 and the byte b belong to different hands."""
    head, nvec, tail, share = cut(align, length)
    body_end = head + 16 * nvec
    out = {head, body_end}
    lanes = set()
    for w in range(REC_NW):                           # a wave's share: its first loads, its tiles' borders, its last loads
        v0, v1 = min(w * share, nvec), min((w + 1) * share, nvec)
        if v0 == v1:
            continue
        lanes.update(range(v0, min(v0 + 3, v1) + 1))
        lanes.update(range(v0, v1 + 1, 64) if v1 - v0 <= 64 * 6 else [v0 + 64, v0 + 128, v1 - (v1 - v0) % 64, v1 - 64])
        lanes.update(range(max(v0, v1 - 2), v1 + 1))
    if nvec <= 130:
        lanes.update(range(nvec + 1))                  # short bodies: every lane border
    out.update(head + 16 * v for v in lanes if 0 <= v <= nvec)
    return sorted(b for b in out if 0 <= b <= length)


# ---- the model -----------------------------------------------------------------------------------------------------------
def positions(data, delim):
    return np.flatnonzero(np.frombuffer(bytes(data), dtype=np.uint8) == delim)


def rec_start(pos, total, r):
    """pos: positions(D, delim), total: len(D)."""
    return 0 if r == 0 else int(pos[r - 1]) + 1 if r <= len(pos) else total


def table_of(pos, out_offs):
    """The record table of an index whose entries start at out_offs: delimiters before every entry, and T."""
    return [int(np.searchsorted(pos, o, side="left")) for o in out_offs] + [len(pos)]


def span_model(table, r):
    n, T = len(table) - 1, table[-1]
    if r == 0:
        return 0, 0
    if r > T:
        return n, 0
    k = min(k for k in range(n) if table[k + 1] >= r)
    return k, r - table[k]


def touched_model(table, lo, cnt):
    """The entries [a, z) that locating and reading records [lo, lo + cnt) need."""
    n = len(table) - 1
    hi = min(lo + cnt, (1 << 64) - 1)
    a = span_model(table, lo)[0] if lo else 0
    if a >= n or hi == 0:
        return 0, 0
    return a, min(span_model(table, hi)[0], n - 1) + 1


def pieces_model(entries, table, ranges):
    blocks = set()
    for lo, cnt in ranges:
        a, z = touched_model(table, lo, cnt)
        blocks |= set(range(a, z))
    out = []
    for k in sorted(blocks):
        lo, hi = entries[k].bit // 8, (entries[k].bit + entries[k].img_bits + 7) // 8 + 8
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi - lo) for lo, hi in out]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def letters(n, seed):
    """n seeded lower-case letters, no two equal neighbours: RLE1 changes nothing, so a level-1 block of libbz2 covers
    99,981 of them."""
    rnd = random.Random(seed)
    out = bytearray(n)
    last = -1
    for i in range(n):
        c = rnd.randrange(25)
        if c >= last:
            c += 1
        if last < 0:
            c = rnd.randrange(26)
        out[i] = 97 + c
        last = c
    return out


BLOCK1 = 99_981                   # raw bytes of a level-1 block without runs


def crafted():
    """350,000 letters with '\\n' planted around the multiples of 99,981: about every 70 bytes before 99,980 and one there;
    at 99,981, a few behind it, at 199,961; at 199,962 only; none behind.  Without the planting, block k of a level-1
    stream covers bytes [99,981 k, 99,981 (k + 1)).  The delimiters at 99,980 / 99,981 and at 199,961 / 199,962 are runs
    of two, and libbz2 never cuts a run: the block that begins one takes it whole.  So the blocks of this input start at 0,
    99,982, 199,963 and 299,944: blocks 0 and 1 END in two delimiters (an empty record on a block's last byte, and a
    record that starts on the next block's first byte), block 1 holds a few inside, blocks 2 and 3 hold none, and the
    unterminated last record covers them both.  An empty record ACROSS a block border would take a run that is cut, that
    is, one of more than 255 delimiters."""
    d = letters(350_000, 11)
    for p in range(69, BLOCK1 - 1, 70):
        d[p] = 10
    for p in (BLOCK1 - 1, BLOCK1, BLOCK1 + 500, BLOCK1 + 501, BLOCK1 + 40_000, 2 * BLOCK1 - 1, 2 * BLOCK1):
        d[p] = 10
    return bytes(d)


def select_js(length, align, seed, nrandom=256):
    """The j list of the all-delimiter content (the answer is j - 1) and the sparse one."""
    js = {1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, length - 1, length, length + 1}
    p = 1
    while p <= length:
        js |= {p - 1, p, p + 1}
        p *= 2
    for b in borders(align, length):
        js |= {b - 1, b, b + 1, b + 2}
    rnd = random.Random(seed)
    js |= {rnd.randrange(1, length + 1) for _ in range(nrandom)} if length else set()
    return sorted(j for j in js if 1 <= j <= length + 1)
