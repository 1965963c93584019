"""The find layer (include/bzx.h: bzx_index_find, bzx_index_get_hits, bzx_find_buffer, bzx_find_geometry, bzx_stage_find).

The rule: the hits of pat in D are find_cases.hits(D, pat) -- every start position, ascending, overlapping ones included;
block, stream, pass, round and window borders do not exist for a hit; only verified bytes count.  The kernels find them
exactly, whatever the alignment, the length and the place of a pattern relative to the borders of find_cases.borders().
CPU part (-m "not gpu"): the kernels, one small multi-block file and the refusals through the fiber emulator (tests/emu).
GPU part (-m gpu): the product library on cuda:0; every input is compressed by Python's bz2 at level 1 (100 MiB of zeros
at level 9, where a block expands to 46.62 MB)."""
import bz2
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import find_cases as FC
import records_cases as RC
from bzx_ctypes import EMU_PATH, LIB_PATH, ROOT
from bzx_find_ctypes import FindLib, IndexInfo, geometry

BZX_OK, BZX_E_PARAM, BZX_E_OUTBUF, BZX_E_STATE, BZX_E_DATA = 0, -2, -4, -6, -7
MiB = 1 << 20


# ---- 1. the kernels through bzx_stage_find ------------------------------------------------------------------------------------
def check_planted(lib, m, shapes, tile, seed=5, max_groups=None):
    """The pattern on and around every border, ending at the segment's end, missing it by one byte on either side (the
    missing byte stands in the neighbouring bytes of the buffer), and near misses, on seeded filler of the same bytes."""
    lay, pat, inside = FC.planted_layout(m, shapes, tile, seed, max_groups)
    counts, allhits = lay.model(pat)
    per = [set(FC.hits(lay.buf[o:o + ln], pat)) for o, ln in lay.segs]
    assert inside and all(s in per[k] for k, s in inside)               # (the plantings are hits of the model)
    rc, got_counts, got = lib.stage_find(lay.buf, lay.segs, pat, 0, len(allhits) + 8)
    assert rc == 0, lib.last_error()
    assert got_counts == counts, [(s, g, w) for s, g, w in zip(lay.segs, got_counts, counts) if g != w][:5]
    assert got == allhits, [(i, g, w) for i, (g, w) in enumerate(zip(got, allhits)) if g != w][:5]
    return len(allhits)


def check_periodic(lib, tile, ms, aligns, big):
    """Period 1 (every position a hit, in the four byte values where a carry or a sign could leak) and period 3."""
    top = (2 * tile + 17 if big else 1040)
    for m in ms:
        lens = [ln for ln in FC.lengths(m, tile, big) if ln <= top]
        segs = [(16 + a, ln) for ln in lens for a in aligns]
        for v in (0x00, 0x7F, 0x80, 0xFF):
            rc, counts, got = lib.stage_find(bytes([v]) * (top + 64), segs, bytes([v]) * m, 0, sum(s[1] for s in segs) + 1)
            assert rc == 0, lib.last_error()
            assert counts == [max(ln - m + 1, 0) for _, ln in segs], (m, v)
            assert got == [p for _, ln in segs for p in range(max(ln - m + 1, 0))], (m, v)
        unit = bytes([0x7F, 0x80, 0xFF])
        buf = unit * ((top + 64) // 3 + 1)
        pat = buf[:m]
        rc, counts, got = lib.stage_find(buf, segs, pat, 0, sum(s[1] for s in segs) + 1)
        want = [FC.hits(buf[o:o + ln], pat) for o, ln in segs]
        assert rc == 0 and counts == [len(w) for w in want] and got == [p for w in want for p in w], m
        assert all(b - a == 3 for w in want for a, b in zip(w, w[1:]))     # (the hits overlap for m > 3)


def check_windows(lib, tile):
    """skip and cap cut the numbering inside a tile, at a tile border, across a segment border and beyond the end; some
    segments are empty."""
    a_len, b_len = 2 * tile + 17, tile + 1
    segs = [(16, 0), (32, a_len), (40, 0), (32 + a_len + 15, b_len), (7, 3)]
    buf = bytes(32 + a_len + 15 + b_len + 64)
    pat = bytes(4)
    na, nb = a_len - 3, b_len - 3
    allhits = list(range(na)) + list(range(nb))
    total = na + nb
    for skip, cap in ((0, 0), (100, 50), (tile - 10, 20), (tile - 3, 1), (tile, 7), (na - 3, 9), (na, 5), (total - 2, 10),
                      (total, 3), (total + 5, 4), (1 << 40, 2), (0, total)):
        rc, counts, got = lib.stage_find(buf, segs, pat, skip, cap)
        assert rc == 0 and counts == [0, na, 0, nb, 0], (skip, cap)
        assert got == allhits[skip:skip + cap], (skip, cap)


def check_stage_refusals(lib):
    assert lib.stage_find(b"abc", [(2, 2)], b"a", 0, 4)[0] == BZX_E_PARAM
    assert "leaves the buffer" in lib.last_error()
    assert lib.stage_find(b"abc", [(0, 3)], b"", 0, 4)[0] == BZX_E_PARAM
    assert lib.stage_find(b"abc", [(0, 3)], None, 0, 4)[0] == BZX_E_PARAM
    assert lib.stage_find(b"abc", [(0, 3)], b"a" * 257, 0, 4)[0] == BZX_E_PARAM
    assert lib.stage_find(b"abc", [], b"a", 0, 4) == (0, [], [])
    assert lib.stage_find(b"abcab", [(0, 5)], b"ab", 0, 4) == (0, [2], [0, 3])


def check_find_refusals(lib, z):
    """bzx_index_find and bzx_index_get_hits: parameters and call order."""
    L = lib.lib
    h = C.c_void_p()
    assert L.bzx_salvage_begin(lib.ctx, 0, C.byref(h)) == 0
    try:
        assert L.bzx_index_find(h, b"ab", 2, 10) == BZX_E_STATE
        assert lib.get_hits(h)[0] == BZX_E_STATE
    finally:
        L.bzx_index_end(h)
    assert L.bzx_index_begin(lib.ctx, 0, C.byref(h)) == 0
    try:
        assert lib.get_hits(h)[0] == BZX_E_STATE and "find was not switched on" in lib.last_error()
        assert L.bzx_index_find(h, None, 2, 10) == BZX_E_PARAM
        assert L.bzx_index_find(h, b"ab", 0, 10) == BZX_E_PARAM and L.bzx_index_find(h, b"a" * 300, 257, 10) == BZX_E_PARAM
        assert L.bzx_index_find(None, b"ab", 2, 10) == BZX_E_PARAM
        assert lib.get_hits(h)[0] == BZX_E_STATE                        # (a refused call switches nothing on)
        assert L.bzx_index_find(h, b"a" * 256, 256, 0) == 0 and L.bzx_index_find(h, b"ab", 2, 10) == 0      # (replaced)
        assert L.bzx_index_count_records(h, 10) == 0
        assert lib.get_hits(h) == (0, [], 0)
        assert L.bzx_index_get_hits(h, None, None, None) == BZX_E_PARAM
        used, done = C.c_size_t(), C.c_int()
        buf = C.create_string_buffer(z[:20], 20)
        assert L.bzx_index_feed(h, C.addressof(buf), 20, 0, C.byref(used), C.byref(done)) == 0
        assert L.bzx_index_find(h, b"ab", 2, 10) == BZX_E_STATE and "before the first" in lib.last_error()
    finally:
        L.bzx_index_end(h)
    info, nl, total = IndexInfo(), C.c_uint64(), C.c_uint64()
    assert L.bzx_find_buffer(lib.ctx, z, len(z), b"", 0, None, 0, C.byref(nl), C.byref(total), None, 0, C.byref(info)) == BZX_E_PARAM
    assert L.bzx_find_buffer(lib.ctx, z, len(z), b"ab", 2, None, 0, None, C.byref(total), None, 0, C.byref(info)) == BZX_E_PARAM
    assert L.bzx_find_buffer(lib.ctx, z, len(z), b"ab", 2, None, 5, C.byref(nl), C.byref(total), None, 0, C.byref(info)) == BZX_E_PARAM


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = FindLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


def test_find_geometry_needs_no_device(emu):
    tile, inline, window = geometry(EMU_PATH)
    assert tile % (FC.WAVES * FC.STEP_BYTES) == 0 and tile >= FC.WAVES * FC.STEP_BYTES and 0 < inline <= window
    emu.lib.bzx_find_geometry.restype = None
    emu.lib.bzx_find_geometry(None, None, None)                         # (every pointer is optional)


@pytest.mark.parametrize("m", FC.M_LIST)
def test_emu_find_kernels_planted(emu, m):
    """The logic of the three kernels on the emulator (a few shapes and plantings; the device runs the whole grid)."""
    tile = geometry(EMU_PATH)[0]
    shapes = [(a, ln) for ln in (0, 1, m - 1, m, m + 1, 17, 1030) for a in (0, 1, 15)] + [(3, tile + 40), (0, 2 * tile + 17)]
    check_planted(emu, m, shapes, tile, max_groups=2)


def test_emu_find_kernels_periodic_and_windows(emu):
    tile = geometry(EMU_PATH)[0]
    check_periodic(emu, tile, (1, 4, 17, 256), (0, 1, 15), big=False)
    check_windows(emu, tile)
    check_stage_refusals(emu)


def small_file():
    """6,000 letters in three small streams with a 17-byte pattern on, at and across the cuts, then 14 streams of one to
    three bytes that spell it once and begin it again -- blocks shorter than the pattern -- and a stream that completes it."""
    cuts = (0, 2500, 4000, 6000)
    pat = bytes(RC.letters(17, 77))
    d = bytearray(RC.letters(cuts[-1], 5))
    for s in (700, 2500 - 17, 2500, 4000 - 8):
        d[s:s + 17] = pat
    d = bytes(d)
    tiny = pat + b"x" + pat[:9]
    pieces, at = [], 0
    while at < len(tiny):
        n = 1 + len(pieces) % 3
        pieces.append(tiny[at:at + n])
        at += n
    raw = d + tiny + pat[9:] + bytes(RC.letters(300, 6))
    z = b"".join(bz2.compress(d[a:b], 1) for a, b in zip(cuts, cuts[1:])) + b"".join(bz2.compress(p, 1) for p in pieces)
    z += bz2.compress(pat[9:] + bytes(RC.letters(300, 6)), 1)
    assert bz2.decompress(z) == raw
    return raw, z, pat


def check_small_file(lib, configs, caps=True):
    raw, z, pat = small_file()
    want = FC.hits(raw, pat)
    assert want == [700, 2500 - 17, 2500, 4000 - 8, 6000, 6018]
    rc, e0, info0 = lib.index_build(z)
    nblk = info0.nblk
    assert rc == 0 and nblk == 18
    offs = [e0[k].out_off for k in range(info0.nblk)] + [len(raw)]
    assert any(any(p < o < p + len(pat) for o in offs) for p in want)                       # across a block border
    assert any(sum(p < o < p + len(pat) for o in offs) >= 3 for p in want)                  # ... across three and more
    rc, hits, total, e, info = lib.find_buffer(z, pat, 100)
    assert rc == 0 and hits == want and total == len(want), lib.last_error()
    assert bytes(info) == bytes(info0) and bytes(e)[:40 * info.nblk] == bytes(e0)[:40 * info.nblk]
    if caps:                                                            # a short list; no index wanted; too little room for it
        rc, hits, total, _, info = lib.find_buffer(z, pat, 3, want_entries=False)
        assert rc == 0 and hits == want[:3] and total == len(want) and info.nblk == nblk
        rc, hits, total, _, info = lib.find_buffer(z, pat, 3, cap_entries=2)
        assert rc == BZX_E_OUTBUF and hits == want[:3] and total == len(want) and info.nblk == nblk
    for feeds, max_chunk in configs:
        rc, keys, info, hrc, hits, total, table, seen = lib.index_feed_find(z, pat, 100, feeds, max_chunk, delim=ord("e"), watch=True)
        assert rc == 0 and hrc == 0 and hits == want and total == len(want), (feeds, max_chunk)
        assert keys == [e0[k].key() for k in range(info0.nblk)] and bytes(info) == bytes(info0)
        assert table == RC.table_of(RC.positions(raw, ord("e")), offs[:-1])
        assert all(a == b[:len(a)] for a, b in zip(seen, seen[1:])) and seen[-1] == want    # a prefix of every later one
    return z


def test_emu_find_small_file(emu):
    z = check_small_file(emu, [(300, 2048)], caps=False)       # (the device runs them: every run decodes 18 blocks here)
    check_find_refusals(emu, z)


# ---- the device ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu16():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = FindLib(max_blocks=16)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def gpu1():
    """One slab: a round is one block."""
    lib = FindLib(max_blocks=1)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def geo():
    return geometry(LIB_PATH)


@pytest.mark.gpu
@pytest.mark.parametrize("m", FC.M_LIST)
def test_gpu_stage_find_planted(gpu16, geo, m):
    tile = geo[0]
    shapes = [(a, ln) for ln in FC.lengths(m, tile) for a in range(16)]
    assert check_planted(gpu16, m, shapes, tile) > len(shapes)


@pytest.mark.gpu
def test_gpu_stage_find_periodic_windows_refusals(gpu16, geo):
    check_periodic(gpu16, geo[0], (1, 2, 3, 4, 5, 16, 17, 255, 256), (0, 1, 15), big=True)
    check_windows(gpu16, geo[0])
    check_stage_refusals(gpu16)


E2E_MS = (2, 17, 256)
FEEDS = [(feeds, chunk) for feeds in (1, 7, 4096) for chunk in (16, 4096)]
# Two kinds of 350,000-byte input.  Seeded letters compress to 50,000 bytes a block; the streaming decoder decodes a block
# that its window does not hold to the end again with every window (a block is withheld until it is complete), so
# 16-byte windows there cost thousands of partial decodes a block (minutes a case on the MI355X): those inputs are fed
# with max_chunk = 4096.  Letters of period 997 compress to about a kilobyte a block, a few dozen 16-byte windows: those
# inputs, with the same plantings around the same block borders, take every combination.
FEEDS_BIG = [(feeds, 4096) for feeds in (1, 7, 4096)]


def planted_file(m, period=None):
    """350,000 letters (seeded, or with `period` the first `period` of them over and over), four level-1 blocks of 99,981,
    with a pattern of m letters on and around the multiples of 99,981: at the first it starts on block 1's first byte
    and ends on block 0's last, at the second it starts one byte before the border and ends one byte before it, at the
    third one byte behind; where room is left it also lies across the border by half."""
    B = RC.BLOCK1
    pat = bytes(RC.letters(m, 100 + m))
    base = bytes(RC.letters(period or 350_000, 21))
    base = (base * (350_000 // len(base) + 1))[:350_000]
    return FC.plant_around(base, pat, [(B, (0, 1, -1)), (2 * B, (-1, 0, 1)), (3 * B, (1, 0, -1))]), pat


def indexed_files(lib, period):
    out = {}
    for m in E2E_MS:
        raw, pat = planted_file(m, period)
        z = bz2.compress(raw, 1)
        rc, e, info = lib.index_build(z)
        assert rc == 0 and info.nblk == 4 and info.out_bytes == len(raw)
        assert [e[k].out_off for k in range(4)] == [k * RC.BLOCK1 for k in range(4)]
        out[m] = (raw, pat, z, e, info, FC.hits(raw, pat))
    return out


@pytest.fixture(scope="module")
def planted(gpu16):
    return indexed_files(gpu16, None)


@pytest.fixture(scope="module")
def planted_periodic(gpu16):
    files = indexed_files(gpu16, 997)
    assert all(len(f[2]) < 16_000 for f in files.values())              # (about a kilobyte a block, and the plantings)
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_find_buffer_planted(gpu16, planted, m):
    raw, pat, z, e0, info0, want = planted[m]
    rc, hits, total, e, info = gpu16.find_buffer(z, pat, len(want) + 5)
    assert rc == 0 and hits == want and total == len(want), gpu16.last_error()
    assert bytes(info) == bytes(info0) and bytes(e)[:160] == bytes(e0)[:160]
    starts = [e[k].out_off for k in range(4)]
    ends = [e[k].out_off + e[k].out_len for k in range(4)]
    assert any(any(p < o < p + m for o in starts[1:]) for p in hits)                        # straddles an entry border
    assert any(p in starts[1:] for p in hits) and any(p + m in ends[:3] for p in hits)      # first byte, last byte
    rc, hits, total, _, _ = gpu16.find_buffer(z, pat, 2, want_entries=False)
    assert rc == 0 and hits == want[:2] and total == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("feeds,max_chunk", FEEDS_BIG)
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_find_fed_in_pieces(gpu1, planted, m, feeds, max_chunk):
    """Small windows and one block a round put window, round and pass borders inside the planted hits."""
    raw, pat, z, e0, info0, want = planted[m]
    delim = ord("e") if (feeds, max_chunk) == FEEDS_BIG[1] else None
    rc, keys, info, hrc, hits, total, table, _ = gpu1.index_feed_find(z, pat, len(want) + 5, feeds, max_chunk, delim=delim)
    assert rc == 0 and hrc == 0, gpu1.why
    assert hits == want and total == len(want)
    assert keys == [e0[k].key() for k in range(4)] and bytes(info) == bytes(info0)
    if delim is not None:                                               # counting on as well: the record table is unchanged
        assert table == RC.table_of(RC.positions(raw, delim), [e0[k].out_off for k in range(4)])


@pytest.mark.gpu
@pytest.mark.parametrize("feeds,max_chunk", FEEDS)
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_find_fed_in_small_windows(gpu1, planted_periodic, m, feeds, max_chunk):
    """max_chunk = 16 and 4096 with pieces of 1, 7 and 4096 bytes over full-size blocks, one slab: window, round and pass
    borders at the block borders, where the plantings start, end and straddle."""
    raw, pat, z, e0, info0, want = planted_periodic[m]
    B = RC.BLOCK1
    assert any(p < k * B < p + m for p in want for k in (1, 2, 3)) and B in want and B - m in want
    rc, keys, info, hrc, hits, total, table, seen = gpu1.index_feed_find(z, pat, len(want) + 5, feeds, max_chunk,
                                                                          delim=ord("e"), watch=True)
    assert rc == 0 and hrc == 0, gpu1.why
    assert hits == want and total == len(want)
    assert keys == [e0[k].key() for k in range(4)] and bytes(info) == bytes(info0)
    assert table == RC.table_of(RC.positions(raw, ord("e")), [k * B for k in range(4)])
    assert all(a == b[:len(a)] for a, b in zip(seen, seen[1:]))


@pytest.mark.gpu
def test_gpu_find_40_tiny_streams(gpu1, gpu16):
    """Streams of one to three bytes: blocks shorter than m - 1, hits across three and more blocks and stream borders."""
    pat = bytes(RC.letters(17, 9))
    text = (pat[5:] + pat + b"q" + pat + pat + pat[:11]) * 2
    pieces, at = [], 0
    for i in range(40):
        n = 1 + (i * 7) % 3
        pieces.append(text[at:at + n])
        at += n
    raw = text[:at]
    z = b"".join(bz2.compress(p, 1) for p in pieces)
    want = FC.hits(raw, pat)
    assert len(want) >= 3 and bz2.decompress(z) == raw
    rc, e0, info0 = gpu16.index_build(z)
    assert rc == 0 and info0.nblk == 40 and info0.nstreams == 40
    for lib in (gpu16, gpu1):
        rc, hits, total, e, info = lib.find_buffer(z, pat, 10)
        assert rc == 0 and hits == want and total == len(want) and bytes(info) == bytes(info0)
        for feeds, max_chunk in FEEDS + [(0, 0)]:
            rc, keys, info, hrc, hits, total, _, seen = lib.index_feed_find(z, pat, 10, feeds, max_chunk, watch=True)
            assert rc == 0 and hits == want and total == len(want), (feeds, max_chunk)
            assert keys == [e0[k].key() for k in range(40)] and bytes(info) == bytes(info0)
            assert all(a == b[:len(a)] for a, b in zip(seen, seen[1:]))


@pytest.mark.gpu
def test_gpu_find_small_file_and_refusals(gpu16):
    z = check_small_file(gpu16, FEEDS)
    check_find_refusals(gpu16, z)


# ---- 3. windows and caps --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zeros():
    return bz2.compress(bytes(100 * MiB), 9)


@pytest.mark.gpu
def test_gpu_find_windows_and_caps(gpu16, geo, zeros):
    tile, inline, window = geo
    N = 100 * MiB
    caps = [0, 1, inline - 1, inline, inline + 1, inline + window + 1]
    if 2 * window + 3 < 4_000_000:
        caps.append(2 * window + 3)
    for cap in caps:
        rc, hits, total, e, info = gpu16.find_buffer(zeros, bytes(4), cap)
        assert rc == 0 and info.nblk == 3 and info.out_bytes == N, gpu16.last_error()
        assert total == N - 3
        assert len(hits) == cap and np.array_equal(np.array(hits, dtype=np.uint64), np.arange(cap, dtype=np.uint64)), cap
    # a window holds at most `window` hits and the inline list `inline`: a list of more than inline + window took the
    # window path more than once
    assert caps[-1] > inline + window
    # a pattern that is not there; and a longer one, whose straddling hits at the two pass borders are more
    rc, hits, total, _, _ = gpu16.find_buffer(zeros, b"\0\0\0\1", 10)
    assert rc == 0 and hits == [] and total == 0
    rc, hits, total, _, _ = gpu16.find_buffer(zeros, bytes(17), 3)
    assert rc == 0 and hits == [0, 1, 2] and total == N - 16


@pytest.mark.gpu
def test_gpu_find_off_means_off(gpu16, planted):
    raw, pat, z, e0, info0, want = planted[17]
    rc, keys, info, hrc, hits, total, _, _ = gpu16.index_feed_find(z, None, 0)
    assert rc == 0 and hrc == BZX_E_STATE and hits is None and "find was not switched on" in gpu16.last_error()
    assert keys == [e0[k].key() for k in range(4)] and bytes(info) == bytes(info0)


# ---- 4. damage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_find_damaged_block(gpu16, gpu1, planted, m):
    raw, pat, z, e0, info0, want = planted[m]
    bad = bytearray(z)
    bad[(e0[2].bit + e0[2].img_bits // 2) // 8] ^= 0x10                 # one payload bit of block 2
    bad = bytes(bad)
    good = e0[2].out_off                                                # the verified prefix: blocks 0 and 1
    want_prefix = FC.hits(raw[:good], pat)
    across = [p for p in want if p < good < p + m]
    assert across and not set(across) & set(want_prefix) and len(want_prefix) < len(want)
    for lib in (gpu16, gpu1):
        rc, hits, total, e, info = lib.find_buffer(bad, pat, len(want) + 5)
        assert rc == BZX_E_DATA
        assert info.nblk == 2 and info.out_bytes == good and bytes(e)[:80] == bytes(e0)[:80]
        assert hits == want_prefix and total == len(want_prefix)
        assert all(p + m <= good for p in hits)
        rc, keys, info, hrc, hits, total, _, _ = lib.index_feed_find(bad, pat, len(want) + 5, 4096, 4096)
        assert rc == BZX_E_DATA and hrc == 0 and hits == want_prefix and total == len(want_prefix) and info.nblk == 2
