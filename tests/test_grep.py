"""The grep layer (include/bzx.h: bzx_index_find_lines, bzx_index_get_hit_lines, bzx_grep_buffer, bzx_stage_find_lines).

The rule: line(p) = the delimiters of D in front of p; for the hit list of bzx_index_get_hits, lines[i] = line(hits[i]),
whatever block, stream, pass, round or window border lies between a delimiter and a hit; grep delivers the records that
hold a listed hit, each once, with their terminating delimiters.  The model is grep_cases (hits from find_cases, lines
from a cumulative count, records from bytes.split).
CPU part (-m "not gpu"): the lines forms of the kernels on a reduced grid, a small multi-stream file, grep and the refusals
through the fiber emulator (tests/emu).  GPU part (-m gpu): the product library on cuda:0."""
import bz2
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import find_cases as FC
import grep_cases as GC
import records_cases as RC
from bzx_ctypes import EMU_PATH, LIB_PATH, ROOT
from bzx_grep_ctypes import GrepLib, geometry

BZX_OK, BZX_E_PARAM, BZX_E_OUTBUF, BZX_E_STATE, BZX_E_DATA = 0, -2, -4, -6, -7
MiB = 1 << 20
NL = 10
DENSE_MS = (1, 2, 3, 4, 5, 17, 256)


# ---- 1. the kernels through bzx_stage_find_lines ---------------------------------------------------------------------------------
def check_segs(lib, buf, segs, pat, delim, what=None):
    """All four results of one call against the model; -> the number of hits."""
    counts, dcounts, hits, lines = GC.seg_model(buf, segs, pat, delim)
    rc, g_counts, g_dcounts, g_hits, g_lines = lib.stage_find_lines(buf, segs, pat, delim, 0, len(hits) + 3)
    assert rc == 0, lib.last_error()
    assert g_counts == counts, (what, [(s, g, w) for s, g, w in zip(segs, g_counts, counts) if g != w][:5])
    assert g_dcounts == dcounts, (what, [(s, g, w) for s, g, w in zip(segs, g_dcounts, dcounts) if g != w][:5])
    assert g_hits == hits, (what, [(i, g, w) for i, (g, w) in enumerate(zip(g_hits, hits)) if g != w][:5])
    assert g_lines == lines, (what, [(i, hits[i], g, w) for i, (g, w) in enumerate(zip(g_lines, lines)) if g != w][:5])
    return len(hits)


def layout(shapes, start=32):
    """Segments of the (align, length) shapes one behind the other, two bytes of other content between them
    -> (buffer length, [(off, len)])"""
    segs, at = [], start
    for align, length in shapes:
        off = at + 2
        off += (align - off) % 16
        segs.append((off, length))
        at = off + length
    return at + 34, segs


def check_dense(lib, m, shapes, delim=NL, seed=3):
    """Seeded bytes over three symbols, the delimiter among them: hits and delimiters on every kind of border.  The
    pattern is a piece of the data itself (the first m bytes of the longest segment), so every m has a hit; for small m
    a third, a ninth, ... of all positions are hits."""
    n, segs = layout(shapes)
    buf = GC.dense(n, seed + m, bytes([delim, 0x61, 0x80]))
    off = max(segs, key=lambda s: s[1])[0]
    pat = buf[off:off + m]
    nh = check_segs(lib, buf, segs, pat, delim, ("dense", m))
    assert nh >= 1
    return nh


def check_cases(lib, tile):
    """The named edges of the issue, small enough for the emulator."""
    sec = tile // 4
    # delim == pat[0]; a pattern that contains the delimiter (the line is that of the hit's first byte)
    n, segs = layout([(a, ln) for ln in (0, 1, 5, 33, 1040) for a in (0, 7, 15)] + [(3, sec + 40)])
    buf = GC.dense(n, 11, b"\nab")
    for pat in (b"\n", b"\na", b"\nab\n", b"a\n", b"ab\n\nb", b"b\n" * 9):
        check_segs(lib, buf, segs, pat, NL, pat)
    assert check_segs(lib, buf, segs, b"a\n", NL) > 100
    # delim == 0 in a buffer of zeros: the zeros that stand for the bytes in front of a head and behind a tail, and the
    # real zeros of the neighbours, never count; every start is a hit and lines[k] == k
    zeros = bytes(n)
    for m in (1, 4, 17):
        rc, counts, dcounts, hits, lines = lib.stage_find_lines(zeros, segs, bytes(m), 0, 0, n)
        assert rc == 0 and dcounts == [ln for _, ln in segs], m
        assert counts == [max(ln - m + 1, 0) for _, ln in segs] and hits == lines == [p for c in counts for p in range(c)], m
    mixed = GC.dense(n, 12, b"\x00\x01\x02")
    for pat in (b"\x00", b"\x01\x00", b"\x02\x02\x00\x01\x01"):
        check_segs(lib, mixed, segs, pat, 0, pat)
    # all-delimiter data with pat = delim x m, in the byte values where a carry or a sign could leak
    for v in (0x0A, 0x7F, 0x80, 0xFF):
        for m in (1, 5):
            rc, counts, dcounts, hits, lines = lib.stage_find_lines(bytes([v]) * n, segs, bytes([v]) * m, v, 0, n)
            assert rc == 0 and dcounts == [ln for _, ln in segs] and hits == lines, (v, m)
            assert hits == [p for _, ln in segs for p in range(max(ln - m + 1, 0))], (v, m)
    # L < m with delimiters present: no hit, the delimiters counted; also where L < m and the run crosses a 16-byte border
    short = [(a, ln) for ln in (1, 2, 16) for a in (0, 9, 15)]
    n2, segs2 = layout(short)
    rc, counts, dcounts, hits, lines = lib.stage_find_lines(b"\n" * n2, segs2, b"\n" * 17, NL, 0, 8)
    assert rc == 0 and counts == [0] * len(short) and dcounts == [ln for _, ln in short] and hits == lines == []
    # delimiters only in the last m - 1 bytes of a segment: in dcounts, in front of no hit; the first of two adjacent
    # segments ends in delimiters and the second one's lines start at 0
    m = 5
    for a, ln in ((0, 64), (5, 1024 + 3), (15, sec + 2), (1, sec - 3)):
        buf2 = bytearray(b"q" * (2 * ln + 64))
        first, second = 16 + a, 16 + a + ln                  # adjacent: the second starts where the first ends
        buf2[first + ln - (m - 1):first + ln] = b"\n" * (m - 1)
        buf2[first:first + m] = buf2[first + ln - 2 * m:first + ln - m] = b"hello"
        buf2[second:second + m] = buf2[second + 7:second + 7 + m] = b"hello"
        buf2[second + 6] = NL
        segs3 = [(first, ln), (second, ln)]
        rc, counts, dcounts, hits, lines = lib.stage_find_lines(bytes(buf2), segs3, b"hello", NL, 0, 8)
        assert rc == 0 and counts == [2, 2] and dcounts == [m - 1, 1], (a, ln)
        assert hits == [0, ln - 2 * m, 0, 7] and lines == [0, 0, 0, 1], (a, ln)
        check_segs(lib, bytes(buf2), segs3, b"hello", NL)


def check_windows(lib, tile):
    """skip and cap cut the numbering inside a step, on a section edge, across a tile edge and a segment border and
    beyond the end: hits and lines stay paired.  Dense data, so the hit numbers of the edges come from the model."""
    sec = tile // 4
    a_len, b_len = 2 * tile + 17, tile + 1
    segs = [(16, 0), (35, a_len), (40, 0), (35 + a_len + 15, b_len), (7, 3)]
    buf = GC.dense(35 + a_len + 15 + b_len + 64, 19, b"\na\x80")
    pat = b"a"
    counts, dcounts, hits, lines = GC.seg_model(buf, segs, pat, NL)
    total, na = len(hits), counts[1]
    assert na > tile // 2 and counts[3] > tile // 8
    below = lambda pos: sum(1 for p in hits[:na] if p < pos)             # hits of segment 1 in front of position pos
    k_sec, k_sec2, k_tile = below(sec - 3), below(2 * sec - 3), below(tile - 3)   # (segment 1 starts 3 bytes behind a border)
    pairs = [(0, 0), (100, 50), (k_sec, k_sec2 - k_sec), (k_sec - 1, 2), (k_tile - 3, 7), (k_tile, 1), (na - 3, 9), (na, 5),
             (total - 2, 10), (total, 3), (total + 5, 4), (1 << 40, 2), (0, total)]
    for skip, cap in pairs:
        rc, g_counts, g_dcounts, g_hits, g_lines = lib.stage_find_lines(buf, segs, pat, NL, skip, cap)
        assert rc == 0 and g_counts == counts and g_dcounts == dcounts, (skip, cap)
        assert g_hits == hits[skip:skip + cap] and g_lines == lines[skip:skip + cap], (skip, cap)


def check_stage_refusals(lib):
    assert lib.stage_find_lines(b"abc", [(2, 2)], b"a", NL, 0, 4)[0] == BZX_E_PARAM and "leaves the buffer" in lib.last_error()
    assert lib.stage_find_lines(b"abc", [(0, 3)], b"", NL, 0, 4)[0] == BZX_E_PARAM
    assert lib.stage_find_lines(b"abc", [(0, 3)], b"a", 256, 0, 4)[0] == BZX_E_PARAM
    assert lib.stage_find_lines(b"abc", [(0, 3)], b"a", -1, 0, 4)[0] == BZX_E_PARAM
    assert lib.stage_find_lines(b"abc", [], b"a", NL, 0, 4) == (0, [], [], [], [])
    assert lib.stage_find_lines(b"ab\nab", [(0, 5)], b"ab", NL, 0, 4) == (0, [2], [1], [0, 3], [0, 1])
    assert lib.stage_find(b"ab\nab", [(0, 5)], b"ab", 0, 4) == (0, [2], [0, 3])            # (the plain forms, as they were)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = GrepLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


@pytest.mark.parametrize("m", (1, 4, 17))
def test_emu_lines_kernels_dense(emu, m):
    """The logic of the three lines forms on the emulator (a reduced grid; the device runs the whole one)."""
    tile = geometry(EMU_PATH)[0]
    shapes = [(a, ln) for ln in list(range(0, 36)) + [1023, 1040] for a in (0, 1, 15)] + [(3, tile // 4 + 40), (0, tile + 17)]
    check_dense(emu, m, shapes)


def test_emu_lines_kernels_cases_and_windows(emu):
    tile = geometry(EMU_PATH)[0]
    check_cases(emu, tile)
    check_windows(emu, tile)
    check_stage_refusals(emu)


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------
def check_lines(lib, raw, z, pat, delim, want_hits, feeds=0, max_chunk=0, rec_delim=NL, max_hits=None):
    """One index pass with find, lines and the record table: lines equal the model, and the record table of the same
    object agrees with them."""
    max_hits = len(want_hits) + 5 if max_hits is None else max_hits
    rc, keys, info, hits, total, lrc, lines, table = lib.index_feed_lines(z, pat, max_hits, delim, feeds, max_chunk, rec_delim)
    assert rc == 0 and lrc == 0, lib.why
    assert hits == want_hits[:max_hits] and total == len(want_hits)
    assert lines == GC.lines_of(raw, hits, delim), (feeds, max_chunk)
    assert all(a <= b for a, b in zip(lines, lines[1:]))
    if rec_delim == delim:
        # keys[k] = (bit, out_off, out_len, ...): the entry k that holds the hit.  rec_before[k] <= line <= rec_before[k + 1]
        # holds always (the upper bound is reached when no delimiter of block k lies at or behind the hit); the exact
        # statement is line = rec_before[k] + the delimiters of block k in front of the hit, and it implies
        # line < rec_before[k + 1] wherever block k has a delimiter at or behind the hit.
        offs = [k[1] for k in keys]
        d = np.frombuffer(raw, dtype=np.uint8)
        for p, line in zip(hits, lines):
            k = int(np.searchsorted(offs, p, side="right")) - 1
            inside = int(np.count_nonzero(d[offs[k]:p] == delim))
            assert table[k] <= line <= table[k + 1] and line == table[k] + inside
            end = offs[k + 1] if k + 1 < len(offs) else len(raw)
            if np.count_nonzero(d[p:end] == delim):
                assert line < table[k + 1]
    return keys, info, hits, lines, table


def small_streams():
    """A text of short lines in three small streams cut inside a line, inside a pattern and on a newline, then 14 streams
    of one to three bytes that hold newlines and spell the pattern across their borders."""
    text, pat = GC.small_text()
    body = (text + b"\n") * 30
    cuts = (0, body.find(b"needle", 500) + 3, body.find(b"\n", 1200) + 1, len(body))
    tiny = b"\nnee\ndle\n\nneedle\n\nneedlen\needle"
    pieces, at = [], 0
    while at < len(tiny):
        n = 1 + len(pieces) % 3
        pieces.append(tiny[at:at + n])
        at += n
    raw = body + tiny
    z = GC.compress_streams([body[a:b] for a, b in zip(cuts, cuts[1:])] + pieces)
    assert bz2.decompress(z) == raw
    return raw, z, pat


def check_small_streams(lib, configs):
    raw, z, pat = small_streams()
    want = FC.hits(raw, pat)
    assert len(want) > 150
    for feeds, max_chunk in configs:
        check_lines(lib, raw, z, pat, NL, want, feeds, max_chunk)
    check_lines(lib, raw, z, b"e\nn", NL, FC.hits(raw, b"e\nn"), *configs[0])             # a pattern that holds the delimiter
    check_lines(lib, raw, z, pat, ord("e"), want, *configs[0], rec_delim=NL)              # the two delimiters are independent
    check_lines(lib, raw, z, pat, NL, want, *configs[0], rec_delim=None, max_hits=7)      # without the table; a short list
    return raw, z, pat


def check_grep(lib, raw, z, pat, delim=NL, max_hits=1 << 20):
    nums, recs = GC.grep(raw, pat, delim)
    total = len(FC.hits(raw, pat))
    assert total <= max_hits
    need = sum(len(r) for r in recs)
    rc, g_nums, g_recs, nrecs, g_need, g_total, trunc = lib.grep_buffer(z, pat, delim, max_hits, len(nums), need)
    assert rc == 0, lib.last_error()
    assert g_nums == nums and g_recs == recs and nrecs == len(nums) and g_need == need and g_total == total and trunc == 0
    return nums, recs, total


def check_grep_small(lib):
    """bzx_grep_buffer on the small text: an empty line, a line with three hits listed once, matches in line 0 and in
    the unterminated last line; both BZX_E_OUTBUF forms; truncation; the refusals; the context afterwards."""
    text, pat = GC.small_text()
    z = bz2.compress(text, 1)
    nums, recs, total = check_grep(lib, text, z, pat)
    assert nums == [0, 3, 5] and total == 5 and recs[0] == b"needle first\n" and recs[2] == b"last needle without an end"
    assert check_grep(lib, text, z, b"first")[0] == [0] and check_grep(lib, text, z, b"no such")[0] == []
    assert check_grep(lib, text, z, b"e", ord("n"))[2] == text.count(b"e")               # another delimiter
    need = sum(len(r) for r in recs)
    rc, _, _, nrecs, g_need, g_total, _ = lib.grep_buffer(z, pat, NL, 100, 2, need)
    assert rc == BZX_E_OUTBUF and nrecs == 3 and g_total == 5 and "cap_recs" in lib.last_error()
    rc, _, _, nrecs, g_need, g_total, _ = lib.grep_buffer(z, pat, NL, 100, 3, need - 1)
    assert rc == BZX_E_OUTBUF and nrecs == 3 and g_need == need
    # truncation: the first two hits are those of lines 0 and 3
    listed = FC.hits(text, pat)[:2]
    t_nums, t_recs = GC.grep(text, pat, NL, listed)
    rc, g_nums, g_recs, nrecs, _, g_total, trunc = lib.grep_buffer(z, pat, NL, 2, 8, 1000)
    assert rc == 0 and g_nums == t_nums == [0, 3] and g_recs == t_recs and g_total == 5 and trunc == 1
    rc, g_nums, _, _, _, g_total, trunc = lib.grep_buffer(z, pat, NL, 5, 8, 1000)
    assert rc == 0 and g_nums == nums and g_total == 5 and trunc == 0
    # refusals
    assert lib.grep_buffer(z, b"need\nle", NL, 100, 8, 1000)[0] == BZX_E_PARAM and "delimiter" in lib.last_error()
    assert lib.grep_buffer(z, b"", NL, 100, 8, 1000)[0] == BZX_E_PARAM
    assert lib.grep_buffer(z, b"x" * 257, NL, 100, 8, 1000)[0] == BZX_E_PARAM
    assert lib.grep_buffer(z, pat, 256, 100, 8, 1000)[0] == BZX_E_PARAM
    assert lib.grep_buffer(b"not a bz2 file at all", pat, NL, 100, 8, 1000)[0] == BZX_E_DATA
    check_grep(lib, text, z, pat)                                       # the context is usable afterwards
    rc, e, info = lib.index_build(z)
    assert rc == 0 and info.out_bytes == len(text)


def check_lines_refusals(lib, z):
    """bzx_index_find_lines and bzx_index_get_hit_lines: parameters and call order."""
    L = lib.lib
    h = C.c_void_p()
    assert L.bzx_salvage_begin(lib.ctx, 0, C.byref(h)) == 0
    try:
        assert L.bzx_index_find_lines(h, NL) == BZX_E_STATE
        assert lib.get_hit_lines(h)[0] == BZX_E_STATE
    finally:
        L.bzx_index_end(h)
    assert L.bzx_index_begin(lib.ctx, 0, C.byref(h)) == 0
    try:
        assert L.bzx_index_find_lines(h, NL) == BZX_E_STATE and "after bzx_index_find" in lib.last_error()      # without find
        assert L.bzx_index_find_lines(None, NL) == BZX_E_PARAM
        assert L.bzx_index_count_records(h, NL) == 0                    # (its order with the record table is free)
        assert L.bzx_index_find(h, b"ab", 2, 10) == 0
        assert lib.get_hit_lines(h)[0] == BZX_E_STATE and "bzx_index_find_lines" in lib.last_error()
        assert L.bzx_index_find_lines(h, 256) == BZX_E_PARAM and L.bzx_index_find_lines(h, -1) == BZX_E_PARAM
        assert lib.get_hit_lines(h)[0] == BZX_E_STATE                   # (a refused call switches nothing on)
        assert L.bzx_index_find_lines(h, 0) == 0 and L.bzx_index_find_lines(h, NL) == 0                         # (replaced)
        assert L.bzx_index_find(h, b"cd", 2, 10) == 0                   # (a new pattern: the lines stay on)
        assert lib.get_hit_lines(h) == (0, [])
        assert L.bzx_index_get_hit_lines(h, None, None) == BZX_E_PARAM
        used, done = C.c_size_t(), C.c_int()
        buf = C.create_string_buffer(z[:20], 20)
        assert L.bzx_index_feed(h, C.addressof(buf), 20, 0, C.byref(used), C.byref(done)) == 0
        assert L.bzx_index_find_lines(h, NL) == BZX_E_STATE and "before the first" in lib.last_error()
    finally:
        L.bzx_index_end(h)


def check_off_means_off(lib, raw, z, pat):
    """Find on, lines off: no lines, and hits, entries and info are those of a run that knows nothing of lines."""
    rc0, hits0, total0, e0, info0 = lib.find_buffer(z, pat, 1 << 16)
    rc, keys, info, hits, total, lrc, lines, table = lib.index_feed_lines(z, pat, 1 << 16, NL, lines=False)
    assert rc == rc0 == 0 and lrc == BZX_E_STATE and lines is None
    assert "lines were not switched on" in lib.lines_why and "bzx_index_find_lines" in lib.lines_why
    assert hits == hits0 == FC.hits(raw, pat) and total == total0
    assert keys == [e0[k].key() for k in range(info0.nblk)] and bytes(info) == bytes(info0)
    # ... and with lines on, the hits, the entries and info are the same again
    rc, keys1, info1, hits1, total1, lrc, lines, _ = lib.index_feed_lines(z, pat, 1 << 16, NL)
    assert rc == 0 and lrc == 0 and keys1 == keys and bytes(info1) == bytes(info0) and hits1 == hits0 and total1 == total0


def test_emu_lines_small_streams(emu):
    raw, z, pat = check_small_streams(emu, [(300, 2048)])
    check_lines_refusals(emu, z)
    check_off_means_off(emu, raw, z, pat)


def test_emu_grep_buffer(emu):
    check_grep_small(emu)
    raw, z, pat = small_streams()
    check_grep(emu, raw, z, pat)


# ---- the device ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu16():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = GrepLib(max_blocks=16)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def gpu1():
    """One slab: a round is one block, so every block is a pass."""
    lib = GrepLib(max_blocks=1)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def geo():
    return geometry(LIB_PATH)


@pytest.mark.gpu
@pytest.mark.parametrize("m", DENSE_MS)
def test_gpu_stage_lines_dense(gpu16, m):
    """Every length 0..96 at every alignment; the lengths within 17 of 1 KiB and 4 KiB at alignments 0, 1 and 15 and of
    16 KiB and 64 KiB at the alignment length mod 16 (all sixteen of them occur); 3 MiB + 5."""
    shapes = [(a, ln) for ln in range(97) for a in range(16)]
    shapes += [(a, c + d) for c in (1024, 4096) for d in range(-17, 18) for a in (0, 1, 15)]
    shapes += [((c + d) % 16, c + d) for c in (16384, 65536) for d in range(-17, 18)]
    check_dense(gpu16, m, shapes)
    check_dense(gpu16, m, [(5, 3 * MiB + 5)], seed=40)


@pytest.mark.gpu
def test_gpu_stage_lines_cases_windows_refusals(gpu16, geo):
    check_cases(gpu16, geo[0])
    check_windows(gpu16, geo[0])
    check_stage_refusals(gpu16)


E2E_MS = (2, 17, 256)
FEEDS = [(feeds, chunk) for feeds in (1, 7, 4096) for chunk in (16, 4096)]


def planted(m, period):
    raw, pat = GC.planted_text(m, period)
    z = bz2.compress(raw, 1)
    B = RC.BLOCK1
    want = FC.hits(raw, pat)
    assert {5001, B, 2 * B - m, 2 * B + 1, 3 * B - m // 2} <= set(want)
    assert raw[B - 1] == NL and raw[2 * B] == NL and raw[3 * B - m // 2 - 1] == NL and raw[3 * B - m // 2 + m] == NL
    return raw, pat, z, want


@pytest.fixture(scope="module")
def files():
    """m -> the seeded file, the periodic file (about a kilobyte a block) and, under "nl", the periodic file whose 17-byte
    pattern holds a newline and straddles the cuts."""
    out = {(m, period): planted(m, period) for m in E2E_MS for period in (None, 997)}
    raw, pat = GC.straddle_text()
    out["nl"] = (raw, pat, bz2.compress(raw, 1), FC.hits(raw, pat))
    B = RC.BLOCK1
    assert out["nl"][3] == [B - 12, 2 * B - 8, 3 * B - 9]
    return out


def check_cuts(keys):
    assert [k[1] for k in keys] == [k * RC.BLOCK1 for k in range(4)]     # the plantings lie where the blocks are cut


@pytest.mark.gpu
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_lines_planted(gpu16, gpu1, files, m):
    """Seeded letters, the whole file in one feed: all blocks in one pass (16 slabs), and every block a pass (one slab)."""
    raw, pat, z, want = files[(m, None)]
    for lib in (gpu16, gpu1):
        keys, info, hits, lines, table = check_lines(lib, raw, z, pat, NL, want)
        check_cuts(keys)
        assert info.out_bytes == len(raw)
    B = RC.BLOCK1
    at = dict(zip(hits, lines))
    assert at[B] == at[5001] + 2 and at[2 * B + 1] == at[2 * B - m] + 1           # the newline on either side of a cut


@pytest.mark.gpu
@pytest.mark.parametrize("feeds,max_chunk", FEEDS)
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_lines_fed_in_small_windows(gpu1, files, m, feeds, max_chunk):
    """One slab, pieces of 1, 7 and 4096 bytes, windows of 16 and 4096: window, round and pass borders at the cuts."""
    raw, pat, z, want = files[(m, 997)]
    assert len(z) < 16_000
    keys, _, _, _, _ = check_lines(gpu1, raw, z, pat, NL, want, feeds, max_chunk)
    check_cuts(keys)


@pytest.mark.gpu
def test_gpu_lines_straddling_hit_with_delimiters_in_the_carry(gpu1, gpu16, files):
    """Every block a pass: the hit that starts 12 bytes in front of the first cut is found on the host, in a carry that
    holds a delimiter in front of its start and one behind it (the pattern's own)."""
    raw, pat, z, want = files["nl"]
    B = RC.BLOCK1
    assert raw[B - 15] == NL and raw[B - 4] == NL and pat[8] == NL
    for lib in (gpu1, gpu16):
        for feeds, max_chunk in ((0, 0), (7, 16), (4096, 4096)):
            keys, _, hits, lines, _ = check_lines(lib, raw, z, pat, NL, want, feeds, max_chunk)
            check_cuts(keys)
            assert lines == [1, 2, 4]


@pytest.mark.gpu
def test_gpu_lines_40_tiny_streams(gpu1, gpu16):
    """Streams of one to three bytes with delimiters among them: passes shorter than m - 1 extend the carry and still add
    their delimiters to the running total."""
    pat = bytes(RC.letters(17, 9))
    text = (pat[5:] + b"\n" + pat + b"\n\nq" + pat + pat[:3] + b"\n" + pat + pat[:11]) * 2
    pieces, at = [], 0
    for i in range(40):
        n = 1 + (i * 7) % 3
        pieces.append(text[at:at + n])
        at += n
    raw = text[:at]
    z = GC.compress_streams(pieces)
    want = FC.hits(raw, pat)
    assert len(want) >= 3 and raw.count(b"\n") >= 4 and bz2.decompress(z) == raw
    for lib in (gpu16, gpu1):
        for feeds, max_chunk in FEEDS + [(0, 0)]:
            keys, info, _, lines, _ = check_lines(lib, raw, z, pat, NL, want, feeds, max_chunk)
            assert info.nblk == 40 and info.nstreams == 40
        check_lines(lib, raw, z, b"\n", NL, FC.hits(raw, b"\n"))         # m == 1, delim == pat[0]: line k for hit k
        check_lines(lib, raw, z, pat[-2:] + b"\n", NL, FC.hits(raw, pat[-2:] + b"\n"), 1, 16)


@pytest.mark.gpu
def test_gpu_lines_small_streams_refusals_off(gpu16, gpu1):
    raw, z, pat = check_small_streams(gpu16, FEEDS + [(0, 0)])
    check_small_streams(gpu1, [(0, 0), (7, 16)])
    check_lines_refusals(gpu16, z)
    check_off_means_off(gpu16, raw, z, pat)


@pytest.mark.gpu
def test_gpu_lines_off_means_off_planted(gpu16, files):
    raw, pat, z, want = files[(17, None)]
    check_off_means_off(gpu16, raw, z, pat)


@pytest.fixture(scope="module")
def zeros():
    return bz2.compress(bytes(100 * MiB), 9)


@pytest.mark.gpu
def test_gpu_lines_zeros_windows(gpu16, geo, zeros):
    """100 MiB of zeros, delim = 0, four zeros: every position is a delimiter and a hit, so lines[i] == hits[i] == i;
    three passes (a level-9 block of zeros expands to 46.62 MB), the inline list and two windows; total is exact."""
    tile, inline, window = geo
    N = 100 * MiB
    for cap in (inline - 1, inline + 1, inline + window + 1):
        rc, keys, info, hits, total, lrc, lines, _ = gpu16.index_feed_lines(zeros, bytes(4), cap, 0)
        assert rc == 0 and lrc == 0 and info.nblk == 3 and info.out_bytes == N and total == N - 3, gpu16.why
        want = np.arange(cap, dtype=np.uint64)
        assert np.array_equal(np.array(hits, dtype=np.uint64), want) and np.array_equal(np.array(lines, dtype=np.uint64), want), cap


@pytest.mark.gpu
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_lines_damaged_block(gpu16, gpu1, files, m):
    raw, pat, z, want = files[(m, None)]
    rc, e0, info0 = gpu16.index_build(z)
    assert rc == 0 and info0.nblk == 4
    bad = bytearray(z)
    bad[(e0[2].bit + e0[2].img_bits // 2) // 8] ^= 0x10                 # one payload bit of block 2
    bad = bytes(bad)
    good = e0[2].out_off                                                # the verified prefix: blocks 0 and 1
    prefix = FC.hits(raw[:good], pat)
    assert 0 < len(prefix) < len(want)
    for lib in (gpu16, gpu1):
        rc, keys, info, hits, total, lrc, lines, table = lib.index_feed_lines(bad, pat, len(want) + 5, NL, rec_delim=NL)
        assert rc == BZX_E_DATA and lrc == 0 and info.nblk == 2 and info.out_bytes == good
        assert hits == prefix and total == len(prefix) and lines == GC.lines_of(raw, prefix, NL)
        assert table == RC.table_of(RC.positions(raw[:good], NL), [0, RC.BLOCK1])
        # grep: the matching records of the prefix, the last one cut at its end
        nums, recs = GC.grep(raw[:good], pat, NL)
        rc, g_nums, g_recs, nrecs, need, g_total, trunc = lib.grep_buffer(bad, pat, NL, 1 << 16, len(nums), sum(map(len, recs)))
        assert rc == BZX_E_DATA and g_nums == nums and g_recs == recs and g_total == len(prefix) and trunc == 0
        assert recs[-1].endswith(pat) and not recs[-1].endswith(b"\n")   # (the pattern that ends on the prefix's last byte)


# ---- 3. bzx_grep_buffer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", E2E_MS)
def test_gpu_grep_buffer_planted(gpu16, gpu1, files, m):
    raw, pat, z, want = files[(m, None)]
    nums, recs, total = check_grep(gpu16, raw, z, pat)
    assert total == len(want) and len(nums) >= 4                        # (two of the planted hits share a line)
    raw, pat, z, want = files[(m, 997)]
    check_grep(gpu1, raw, z, pat)


@pytest.mark.gpu
def test_gpu_grep_buffer_small_text(gpu16, gpu1):
    check_grep_small(gpu16)
    check_grep_small(gpu1)
    raw, z, pat = small_streams()
    check_grep(gpu16, raw, z, pat)
