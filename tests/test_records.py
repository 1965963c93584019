"""The record layer (include/bzx.h: bzx_index_count_records, bzx_records_*, bzx_decompress_records_*, bzx_stage_rec_*).

The rules: the record table counts the delimiters before every block; byte_offs of a locate call are rec_start(r) of
np.flatnonzero(D == delim); records [lo, lo + cnt) are D[rec_start(lo), rec_start(lo + cnt)); a damaged block, a stale
entry or a stale count fails exactly what touches it; the two kernels count and select exactly, whatever the alignment,
the length and the place of a delimiter relative to the borders of records_cases.borders().
CPU part (-m "not gpu"): the host-only planners on crafted tables, the .bzxr layout, and the kernels and one small file
through the fiber emulator (tests/emu).  GPU part (-m gpu): the product library on cuda:0; every input is compressed by
Python's bz2 at level 1 (100 MiB of zeros at level 9, where a block expands to 46.62 MB)."""
import bz2
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import records_cases as RC
from bzx_ctypes import EMU_PATH, LIB_PATH, ROOT
from bzx_records_ctypes import NONE, IndexEntry, IndexInfo, RecordsLib, pack_bzxr, planners, read_bzxr, u64

BZX_OK, BZX_E_PARAM, BZX_E_OUTBUF, BZX_E_STATE, BZX_E_DATA = 0, -2, -4, -6, -7
MiB = 1 << 20


# ---- 1. the planners: host only ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    if not os.path.exists(LIB_PATH):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return planners()


def fake_entries(n, img_bits=8000, gap_bits=0):
    """n entries of 1000 decoded bytes whose images lie back to back behind a 4-byte header."""
    e = (IndexEntry * max(n, 1))()
    bit = 32
    for k in range(n):
        e[k].bit, e[k].out_off, e[k].out_len, e[k].img_bits, e[k].level = bit, 1000 * k, 1000, img_bits, 1
        bit += img_bits + gap_bits
    return e


TABLES = {
    "empty_index": [0],
    "one_block": [0, 5],
    "zeros_front": [0, 0, 0, 3, 7],
    "zeros_middle": [0, 4, 4, 4, 9, 9, 12],
    "zeros_end": [0, 2, 6, 6, 6],
    "all_zero": [0, 0, 0, 0],
    "past_2_32": [0, (1 << 32) - 2, (1 << 32) + 5, (1 << 33) + 1, (1 << 33) + 1, (1 << 34)],
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_records_span_against_the_model(plan, name):
    table = TABLES[name]
    T = table[-1]
    rs = {0, 1, 2, T - 1, T, T + 1, 1 << 63, (1 << 64) - 1} | {v + d for v in table for d in (-1, 0, 1)}
    for r in sorted(x for x in rs if 0 <= x < 1 << 64):
        rc, entry, j = plan.span(table, r)
        assert rc == BZX_OK and (entry, j) == RC.span_model(table, r), (name, r)
        if j:
            assert 1 <= j <= table[entry + 1] - table[entry]


def test_records_span_refusals(plan):
    assert plan.span([1, 2, 3], 1)[0] == BZX_E_PARAM                    # rec_before[0] != 0
    assert plan.span([0, 5, 4, 9], 1)[0] == BZX_E_PARAM                 # descends
    assert plan.span([0, 5, 9, 8], 1)[0] == BZX_E_PARAM                 # ... at the end
    assert plan.span(None, 1, n=0)[0] == BZX_E_PARAM
    assert plan.lib.bzx_records_span(u64([0, 1]), 1, 1, None, None) == BZX_E_PARAM


@pytest.mark.parametrize("name", sorted(TABLES))
def test_records_pieces_against_the_model(plan, name):
    table = TABLES[name]
    n, T = len(table) - 1, table[-1]
    for gap_bits in (0, 200_000):                                       # adjacent images merge, distant ones do not
        e = fake_entries(n, gap_bits=gap_bits)
        edges = sorted({0, 1, 2, T - 1, T, T + 1, 1 << 63} | {v + d for v in table for d in (-1, 0, 1)})
        edges = [x for x in edges if 0 <= x < 1 << 64]
        cases = [[(lo, cnt)] for lo in edges for cnt in (0, 1, 2, T, (1 << 64) - 1)]
        rnd = random.Random(7)
        cases += [[(rnd.choice(edges), rnd.choice((0, 1, 3, T))) for _ in range(rnd.randrange(0, 6))] for _ in range(40)]
        for ranges in cases:
            want = RC.pieces_model(e, table, ranges)
            rc, got, np_ = plan.pieces(e, n, table, ranges, cap=n + 2)
            assert rc == BZX_OK and np_ == len(want) and got == want, (name, gap_bits, ranges)
            if len(want) > 1:                                           # too little room: the count, and the first ones
                rc, got, np_ = plan.pieces(e, n, table, ranges, cap=1)
                assert rc == BZX_E_OUTBUF and np_ == len(want) and got == want[:1]


def test_records_pieces_refusals(plan):
    e = fake_entries(3)
    assert plan.pieces(e, 3, [0, 2, 1, 5], [(0, 1)])[0] == BZX_E_PARAM
    assert plan.pieces(e, 3, [1, 2, 3, 5], [(0, 1)])[0] == BZX_E_PARAM
    assert plan.lib.bzx_records_pieces(e, 3, u64([0, 1, 2, 3]), 1, None, None, None, None, 0, C.byref(C.c_uint32())) == BZX_E_PARAM


def test_bzxr_layout_both_directions(tmp_path):
    table = [0, 3, 3, (1 << 32) + 7]
    raw = pack_bzxr(10, table)
    assert raw[:4] == b"BZXR" and len(raw) == 32 + 8 * 4
    assert raw[4:8] == b"\x01\0\0\0" and raw[8:12] == b"\x0a\0\0\0" and raw[12:16] == bytes(4)
    assert raw[16:24] == (3).to_bytes(8, "little") and raw[24:32] == ((1 << 32) + 7).to_bytes(8, "little")
    assert raw[32:] == b"".join(v.to_bytes(8, "little") for v in table)
    p = tmp_path / "x.bz2.bzxr"
    p.write_bytes(raw)
    assert read_bzxr(str(p)) == (10, table)
    p.write_bytes(pack_bzxr(0, [0]))                                    # the empty index
    assert read_bzxr(str(p)) == (0, [0]) and p.stat().st_size == 40


# ---- 2. the kernels through the stage entries -------------------------------------------------------------------------------
def fillers(delim):
    return bytes([delim ^ 1, delim ^ 0x80])


def kernel_shapes(big):
    """(length, alignments)"""
    shapes = [(ln, range(16)) for ln in range(97)]
    shapes += [(ln, (0, 1, 15)) for ln in (255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537)]
    if big:
        shapes.append((3 * MiB + 5, (0, 1, 15)))
    return shapes


def check_uniform(lib, delim, shapes):
    """Every byte the delimiter: the count is the length.  No byte the delimiter, every byte next to it: the count is 0."""
    top = max(ln for ln, _ in shapes) + 32
    segs = [(a, ln) for ln, aligns in shapes for a in aligns]
    rc, got = lib.stage_count(bytes([delim]) * top, segs, delim)
    assert rc == 0, lib.last_error()
    assert got == [ln for _, ln in segs], [(s, g) for s, g in zip(segs, got) if g != s[1]][:5]
    rc, got = lib.stage_count((fillers(delim) * (top // 2 + 1))[:top], segs, delim)
    assert rc == 0 and got == [0] * len(segs), [(s, g) for s, g in zip(segs, got) if g][:5]
    # the select kernel on the same two contents: the count, and none to find
    qs = [(a, ln, 1) for a, ln in segs]
    rc, pos, cnt = lib.stage_select((fillers(delim) * (top // 2 + 1))[:top], qs, delim)
    assert rc == 0 and cnt == [0] * len(qs) and pos == [NONE] * len(qs)


def check_single(lib, delim, shapes):
    """One delimiter alone at b - 1 and at b, for every border b: windows of one buffer that holds two delimiters, one at
    an address that is 0 mod 16 and one at 15 mod 16, further apart than the longest window."""
    top = max(ln for ln, _ in shapes)
    span = (top + 64) & ~15
    buf = bytearray((fillers(delim) * (2 * span + 32))[:4 * span + 64])
    d0, d1 = span, 3 * span + 15                     # a window [d - b, + length) sees align + head = 0 mod 16
    buf[d0] = buf[d1] = delim
    qs, want = [], []
    for ln, aligns in shapes:
        for a in aligns:
            for b in RC.borders(a, ln):
                for at in (b - 1, b):
                    if not 0 <= at < ln:
                        continue
                    d = d0 if (a + at) % 16 == 0 else d1
                    if (d - at) % 16 != a:
                        continue                     # (borders lie at a + b = 0 mod 16: one of the two always serves)
                    qs.append((d - at, ln, 1))
                    want.append(at)
    assert len(qs) > len(shapes)
    rc, got = lib.stage_count(bytes(buf), [(o, ln) for o, ln, _ in qs], delim)
    assert rc == 0 and got == [1] * len(qs), [(q, g) for q, g in zip(qs, got) if g != 1][:5]
    rc, pos, cnt = lib.stage_select(bytes(buf), qs, delim)
    assert rc == 0 and cnt == [1] * len(qs)
    assert pos == want, [(q, p, w) for q, p, w in zip(qs, pos, want) if p != w][:5]


def check_select_all(lib, delim, shapes, nrandom=256, many=700):
    """Every byte the delimiter: delimiter j is byte j - 1; j = length + 1 finds none."""
    top = max(ln for ln, _ in shapes) + 32
    qs = []
    for ln, aligns in shapes:
        for a in aligns:
            qs += [(a, ln, j) for j in RC.select_js(ln, a, 1000 * ln + a, nrandom)] + [(a, ln, 0)]
    ln, a = shapes[-1][0], 1
    qs += [(a, ln, j) for j in range(1, min(ln, many) + 1)] + [(a, ln, max(ln // 2, 1))] * 3      # many on one segment, one thrice
    rc, pos, cnt = lib.stage_select(bytes([delim]) * top, qs, delim)
    assert rc == 0, lib.last_error()
    assert cnt == [ln for _, ln, _ in qs]
    want = [j - 1 if 1 <= j <= ln else NONE for _, ln, j in qs]
    assert pos == want, [(q, p, w) for q, p, w in zip(qs, pos, want) if p != w][:5]


def check_select_sparse(lib, delim, shapes, nrandom=256):
    """Seeded content of density 1/64 against the model, with j = 0 and j = count + 1."""
    top = max(ln for ln, _ in shapes) + 32
    rnd = np.random.default_rng(delim + 17)
    a_ = np.frombuffer((fillers(delim) * (top // 2 + 1))[:top], dtype=np.uint8).copy()
    a_[rnd.random(top) < 1 / 64] = delim
    where = np.flatnonzero(a_ == delim)
    qs, want_pos, want_cnt = [], [], []
    for ln, aligns in shapes:
        for a in aligns:
            lo, hi = np.searchsorted(where, a), np.searchsorted(where, a + ln)
            count = int(hi - lo)
            js = {0, count + 1} | {j for j in RC.select_js(ln, a, 77 * ln + a, nrandom) if j <= count}
            for j in sorted(js):
                qs.append((a, ln, j))
                want_cnt.append(count)
                want_pos.append(int(where[lo + j - 1]) - a if 1 <= j <= count else NONE)
    rc, pos, cnt = lib.stage_select(a_.tobytes(), qs, delim)
    assert rc == 0 and cnt == want_cnt
    assert pos == want_pos, [(q, p, w) for q, p, w in zip(qs, pos, want_pos) if p != w][:5]
    rc, got = lib.stage_count(a_.tobytes(), [(a, ln) for ln, aligns in shapes for a in aligns], delim)
    assert rc == 0 and got == [int(np.searchsorted(where, a + ln) - np.searchsorted(where, a)) for ln, aligns in shapes for a in aligns]


def check_stage_refusals(lib):
    assert lib.stage_count(b"abc", [(2, 2)], 10)[0] == BZX_E_PARAM
    assert lib.stage_count(b"abc", [(0, 3)], 256)[0] == BZX_E_PARAM
    assert lib.stage_select(b"abc", [(4, 0, 1)], 10)[0] == BZX_E_PARAM
    assert lib.stage_count(b"a\nc", [], 10) == (0, [])


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = RecordsLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


EMU_SHAPES = [(ln, (0, 1, 7, 15)) for ln in (0, 1, 15, 16, 17, 33, 96)] + [(4097, (0, 15)), (70_001, (3,))]


def test_emu_record_kernels(emu):
    """The logic of the two kernels on the emulator (a few shapes; the device runs the whole grid)."""
    for delim in (0x0A, 0x80):
        check_uniform(emu, delim, EMU_SHAPES)
        check_single(emu, delim, EMU_SHAPES)
    check_select_all(emu, 0x80, EMU_SHAPES[:8], nrandom=8, many=40)
    check_select_sparse(emu, 0x0A, EMU_SHAPES, nrandom=8)
    check_stage_refusals(emu)


SMALL_CUTS = (0, 2500, 4000, 6000)


def small_file():
    """Three small blocks of letters with a few lines, as three concatenated streams (the emulator decodes them)."""
    d = bytearray(RC.letters(SMALL_CUTS[-1], 5))
    for p in (0, 7, 8, 1200, 2499, 2500, 3100, 5999):
        d[p] = 10
    d = bytes(d)
    return d, b"".join(bz2.compress(d[a:z], 1) for a, z in zip(SMALL_CUTS, SMALL_CUTS[1:]))


def check_small_file(lib):
    raw, z = small_file()
    pos = RC.positions(raw, 10)
    rc, e, info, table = lib.index_records(z, 10)
    n = info.nblk
    assert rc == 0 and n == 3 and table == RC.table_of(pos, [e[k].out_off for k in range(n)])
    recs = list(range(0, len(pos) + 3)) + [1 << 63]
    rc, offs, st = lib.locate_buffer(z, None, e, n, table, 10, recs)
    assert rc == 0 and st == [0] * len(recs), lib.last_error()
    assert offs == [RC.rec_start(pos, len(raw), r) for r in recs]
    ranges = [(0, 1), (1, 2), (3, 0), (2, 5), (len(pos), 1), (len(pos) + 1, 4), (0, 1 << 64 - 1), (2, 5)]
    want = [raw[RC.rec_start(pos, len(raw), lo):RC.rec_start(pos, len(raw), min(lo + c, (1 << 64) - 1))] for lo, c in ranges]
    rc, pieces, np_ = lib.pieces(e, n, table, ranges)
    assert rc == 0 and pieces == RC.pieces_model(e, table, ranges)
    r = lib.records_buffer(z, pieces, e, n, table, 10, ranges, sum(map(len, want)))
    assert r.rc == 0 and r.status == [0] * len(ranges), lib.last_error()
    assert [r.data(i) for i in range(len(ranges))] == want and r.need == sum(map(len, want))
    # a count moved from block 0 to block 1: block 0's queries fail, block 2's do not
    stale = list(table)
    stale[1] -= 1
    rc, offs, st = lib.locate_buffer(z, None, e, n, stale, 10, [1, len(pos)])
    assert rc == BZX_E_DATA and st == [BZX_E_DATA, 0] and offs[1] == RC.rec_start(pos, len(raw), len(pos))
    assert "record table does not match the input: block 0 holds" in lib.last_error()


def test_emu_records_small_file(emu):
    check_small_file(emu)


@pytest.fixture(scope="module")
def gpu16():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = RecordsLib(max_blocks=16)
    yield lib
    lib.close()


@pytest.mark.gpu
@pytest.mark.parametrize("delim", RC.DELIMS)
def test_gpu_count_and_select_grid(gpu16, delim):
    shapes = kernel_shapes(big=True)
    check_uniform(gpu16, delim, shapes)
    check_single(gpu16, delim, shapes)


@pytest.mark.gpu
@pytest.mark.parametrize("delim", RC.DELIMS)
def test_gpu_select_all_delimiters(gpu16, delim):
    check_select_all(gpu16, delim, [(ln, (0, 1, 15)) for ln in (0, 1, 2, 15, 16, 17, 31, 33, 64, 96, 255, 256, 257, 4095, 4096, 4097,
                                                               65535, 65536, 65537, 3 * MiB + 5)])


@pytest.mark.gpu
@pytest.mark.parametrize("delim", RC.DELIMS)
def test_gpu_select_sparse(gpu16, delim):
    check_select_sparse(gpu16, delim, [(ln, (0, 1, 15)) for ln in (0, 1, 17, 96, 257, 4097, 65537, 3 * MiB + 5)])
    check_stage_refusals(gpu16)


# ---- 3. end to end on the device ---------------------------------------------------------------------------------------------
def build_table(lib, z, delim, raw, nblk=None):
    """The index with counting on, held against the model -> (entries, n, table, positions)."""
    pos = RC.positions(raw, delim)
    rc, e, info, table = lib.index_records(z, delim)
    assert rc == 0, lib.last_error()
    n = info.nblk
    assert info.out_bytes == len(raw) and (nblk is None or n == nblk)
    assert table == RC.table_of(pos, [e[k].out_off for k in range(n)])
    return e, n, table, pos


def want_records(raw, pos, ranges):
    return [raw[RC.rec_start(pos, len(raw), lo):RC.rec_start(pos, len(raw), min(lo + c, (1 << 64) - 1))] for lo, c in ranges]


def check_read(lib, z, e, n, table, delim, raw, pos, ranges, pieces="model"):
    want = want_records(raw, pos, ranges)
    pcs = RC.pieces_model(e, table, ranges) if pieces == "model" else pieces
    r = lib.records_buffer(z, pcs, e, n, table, delim, ranges, sum(map(len, want)))
    assert r.rc == 0 and r.status == [0] * len(ranges), lib.last_error()
    assert r.need == sum(map(len, want)) and r.gots == [len(w) for w in want]
    for i, w in enumerate(want):
        assert r.data(i) == w, (i, ranges[i])


@pytest.fixture(scope="module")
def crafted(gpu16):
    raw = RC.crafted()
    z = bz2.compress(raw, 1)
    e, n, table, pos = build_table(gpu16, z, 10, raw)
    return raw, z, e, n, table, pos


@pytest.mark.gpu
def test_gpu_crafted_edges(gpu16, crafted):
    raw, z, e, n, table, pos = crafted
    B = RC.BLOCK1
    # RLE1 changes nothing here, so a block takes 99,981 bytes -- and the whole of a run that it has begun: the two
    # delimiters planted on the last byte of one block and the first of the next are a run of two, which libbz2 never
    # cuts, so blocks 0 and 1 end one byte later than a multiple of 99,981 and hold both (records_cases.crafted)
    assert n == 4 and [e[k].out_off for k in range(4)] == [0, B + 1, 2 * B + 1, 3 * B + 1]
    T = len(pos)
    assert table[2] == table[3] == table[4] == T and raw[B - 1] == raw[B] == raw[2 * B - 1] == raw[2 * B] == 10
    recs = {0, 1, 2, T - 1, T, T + 1, T + 2, 1 << 63}
    for k in range(1, 4):
        recs |= {table[k] + d for d in (-1, 0, 1, 2)}
    recs = sorted(r for r in recs if r >= 0)
    rc, offs, st = gpu16.locate_buffer(z, None, e, n, table, 10, recs)
    assert rc == 0 and st == [0] * len(recs), gpu16.last_error()
    assert offs == [RC.rec_start(pos, len(raw), r) for r in recs]
    # a record that starts on a block's first byte (twice), an empty record that ends on a block's last byte (twice; it
    # cannot lie across a border, see above), the unterminated tail over two blocks
    assert RC.rec_start(pos, len(raw), table[1]) == B + 1 == e[1].out_off and RC.rec_start(pos, len(raw), table[1] - 1) == B
    assert RC.rec_start(pos, len(raw), T) == 2 * B + 1 == e[2].out_off and RC.rec_start(pos, len(raw), T - 1) == 2 * B
    assert want_records(raw, pos, [(table[1] - 1, 1), (T - 1, 1)]) == [b"\n", b"\n"]
    assert len(want_records(raw, pos, [(T, 1)])[0]) == len(raw) - 2 * B - 1 > B
    in_order = [(r, 2) for r in range(0, T + 2, 97)]
    rnd = random.Random(3)
    shuffled = in_order[:]
    rnd.shuffle(shuffled)
    edge = [(table[1] - 1, 1), (table[1], 1), (table[1] - 1, 3), (table[2] - 1, 1), (table[2], 1), (T - 1, 1), (T, 1), (T, 5),
            (T - 1, 9), (0, 1), (0, 0), (5, 0), (T + 1, 3), (1 << 63, 1 << 63), (0, T + 1), (10, 1), (10, 1), (8, 5), (9, 4)]
    for ranges in (in_order, shuffled, edge, edge + shuffled[:9]):
        check_read(gpu16, z, e, n, table, 10, raw, pos, ranges)
        check_read(gpu16, z, e, n, table, 10, raw, pos, ranges, pieces=None)
    rc, pieces, np_ = gpu16.pieces(e, n, table, edge, cap=8)
    assert rc == 0 and pieces == RC.pieces_model(e, table, edge)
    # the pieces are needed: without the last block's bytes the tail record is refused as a whole-call error
    r = gpu16.records_buffer(z, [(0, e[3].bit // 8)], e, n, table, 10, [(T, 1)], 200_000)
    assert r.rc == BZX_E_PARAM and r.status == [BZX_E_PARAM]


@pytest.mark.gpu
def test_gpu_empty_records_across_a_block_border(gpu16):
    """A run that libbz2 does cut: 99,978 letters and 300 delimiters.  RLE1 writes the first 255 of them as five bytes, which
    fill block 0 (99,983 >= 99,981); block 1 starts with the other 45.  The empty records around the border have one
    boundary in each block."""
    L = 99_978
    raw = bytes(RC.letters(L, 13)) + b"\n" * 300 + bytes(RC.letters(50_000, 14))
    z = bz2.compress(raw, 1)
    e, n, table, pos = build_table(gpu16, z, 10, raw, nblk=2)
    assert e[1].out_off == L + 255 and table == [0, 255, 300]
    recs = list(range(250, 262)) + [299, 300, 301]
    rc, offs, st = gpu16.locate_buffer(z, None, e, n, table, 10, recs)
    assert rc == 0 and st == [0] * len(recs) and offs == [RC.rec_start(pos, len(raw), r) for r in recs]
    ranges = [(254, 1), (255, 1), (256, 1), (254, 3), (0, 1), (300, 1), (250, 60)]
    assert want_records(raw, pos, ranges)[:3] == [b"\n"] * 3
    check_read(gpu16, z, e, n, table, 10, raw, pos, ranges)


@pytest.mark.gpu
def test_gpu_crafted_device_forms(gpu16, crafted):
    import torch
    raw, z, e, n, table, pos = crafted
    T = len(pos)
    d_z = torch.empty(len(z) + 16, dtype=torch.uint8, device="cuda")
    d_z[3:3 + len(z)] = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    from bzx_ranges_ctypes import Piece
    pc = (Piece * 1)(Piece(d_z.data_ptr() + 3, 0, len(z)))
    recs = [0, 1, table[1], table[1] + 1, table[2] + 1, T, T + 1]
    rc, offs, st = gpu16.locate_raw(gpu16.lib.bzx_records_locate_device, pc, 1, e, n, table, 10, recs)
    assert rc == 0 and st == [0] * len(recs) and offs == [RC.rec_start(pos, len(raw), r) for r in recs]
    ranges = [(table[1] - 1, 3), (T, 1), (0, 2), (table[1] - 1, 3)]
    want = want_records(raw, pos, ranges)
    need = sum(map(len, want))
    d_o = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = gpu16.records_raw(gpu16.lib.bzx_decompress_records_device, pc, 1, e, n, table, 10, ranges, d_o.data_ptr() + 1, need)
    torch.cuda.synchronize()
    back = d_o.cpu().numpy().tobytes()
    assert r.rc == 0 and r.need == need and back[1:1 + need] == b"".join(want) and back[0] == 0xA5 and back[1 + need] == 0xA5
    d_raw = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    out = u64([0] * (n + 1))
    assert gpu16.lib.bzx_records_count_device(gpu16.ctx, d_raw.data_ptr(), len(raw), 10, e, n, out) == 0
    assert list(out[:n + 1]) == table


@pytest.mark.gpu
def test_gpu_more_inputs(gpu16):
    rnd = random.Random(9)
    words = bytes(RC.letters(30_000, 2))
    lines = b"".join(words[i:i + rnd.randrange(1, 90)] + b"\n" for i in range(0, 29_000, 53))
    # three concatenated streams: one empty, one without a delimiter, one ordinary
    raw = words[:5000] + lines
    z = bz2.compress(b"", 1) + bz2.compress(words[:5000], 1) + bz2.compress(lines, 1)
    e, n, table, pos = build_table(gpu16, z, 10, raw, nblk=2)
    assert table[1] == 0
    T = len(pos)
    check_read(gpu16, z, e, n, table, 10, raw, pos, [(0, 1), (1, 1), (T - 1, 1), (T, 1), (T - 3, 9), (0, T + 1)])
    # ends in the delimiter: record T is empty
    assert raw.endswith(b"\n") and want_records(raw, pos, [(T, 1)]) == [b""]
    # none
    z0 = bz2.compress(words, 1)
    e0, n0, t0, p0 = build_table(gpu16, z0, 10, words, nblk=1)
    assert t0 == [0, 0]
    check_read(gpu16, z0, e0, n0, t0, 10, words, p0, [(0, 1), (0, 0), (1, 1), (0, 2)])
    rc, offs, st = gpu16.locate_buffer(z0, [], e0, n0, t0, 10, [0, 1, 2])      # no query needs the device, or a piece
    assert rc == 0 and offs == [0, len(words), len(words)]
    # the empty input
    ze = bz2.compress(b"", 1)
    rc, ee, info, te = gpu16.index_records(ze, 10)
    assert rc == 0 and info.nblk == 0 and te == [0]
    rc, offs, st = gpu16.locate_buffer(ze, [], ee, 0, te, 10, [0, 1, 1 << 63])
    assert rc == 0 and offs == [0, 0, 0] and st == [0, 0, 0]
    r = gpu16.records_buffer(ze, [], ee, 0, te, 10, [(0, 5), (3, 1)], 0)
    assert r.rc == 0 and r.gots == [0, 0] and r.need == 0


@pytest.mark.gpu
@pytest.mark.parametrize("delim", (0x00, 0xFF))
def test_gpu_runs_of_delimiters(gpu16, delim):
    """Binary data with runs of 300 delimiter bytes: the counts go through the RLE1 expansion."""
    rnd = random.Random(delim + 1)
    parts = []
    for i in range(400):
        parts.append(bytes(rnd.randrange(1, 255) for _ in range(rnd.randrange(1, 700))).replace(bytes([delim]), b"\x55"))
        parts.append(bytes([delim]) * (300 if i % 3 else rnd.randrange(1, 9)))
    raw = b"".join(parts)
    z = bz2.compress(raw, 1)
    e, n, table, pos = build_table(gpu16, z, delim, raw)
    assert n >= 2 and len(pos) > 80_000
    T = len(pos)
    ranges = [(0, 1), (299, 3), (T // 2, 400), (T - 1, 1), (T, 1)] + [(rnd.randrange(T), rnd.randrange(4)) for _ in range(40)]
    check_read(gpu16, z, e, n, table, delim, raw, pos, ranges)


@pytest.mark.gpu
def test_gpu_100_mib_of_zeros(gpu16):
    total = 100 * MiB
    z = bz2.compress(bytes(total), 9)           # (level 9: 900,000 x 259 / 5 bytes a block, so three blocks and counts above 2^25)
    rc, e, info, table = gpu16.index_records(z, 0)
    n = info.nblk
    assert rc == 0 and n == 3 and info.out_bytes == total, gpu16.last_error()
    assert min(e[k].out_len for k in range(2)) > 1 << 25
    assert table == [e[k].out_off for k in range(n)] + [total]
    recs = [0, 1, e[1].out_off, e[1].out_off + 1, e[2].out_off + 5, total, total + 1]
    rc, offs, st = gpu16.locate_buffer(z, None, e, n, table, 0, recs)
    assert rc == 0 and offs == [min(r, total) for r in recs]


@pytest.mark.gpu
def test_gpu_two_rounds_fed_in_small_pieces(gpu16):
    raw = bytearray(RC.letters(2_100_000, 4))
    rnd = random.Random(6)
    for _ in range(30_000):
        raw[rnd.randrange(len(raw))] = 10
    raw = bytes(raw)
    z = bz2.compress(raw, 1)
    e, n, table, pos = build_table(gpu16, z, 10, raw, nblk=22)
    rc, keys, info, fed = gpu16.index_feed_records(z, 10, feeds=1024, max_chunk=64 << 10)
    assert rc == 0 and info.nblk == 22 and fed == table
    assert keys == [e[k].key() for k in range(n)]


# ---- 4. contracts -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_counting_off_means_off(gpu16, crafted):
    raw, z, e, n, table, pos = crafted
    rc, keys, info, rrc = gpu16.index_feed_records(z, None)
    assert rc == 0 and rrc == BZX_E_STATE and "counting was not switched on" in gpu16.last_error()
    rc, e_off, info_off = gpu16.index_build(z)
    assert rc == 0 and info_off.nblk == n
    assert bytes(e_off)[:40 * n] == bytes(e)[:40 * n] and keys == [e[k].key() for k in range(n)]
    rc2, e_on, info_on, _ = gpu16.index_records(z, 10)
    assert bytes(info_on) == bytes(info_off)
    # too little room: the first entries, their table, the count needed
    rc, e2, info2, t2 = gpu16.index_records(z, 10, cap=2)
    assert rc == BZX_E_OUTBUF and info2.nblk == n and t2 == table[:3] and bytes(e2)[:80] == bytes(e)[:80]
    assert gpu16.lib.bzx_index_build_records_buffer(gpu16.ctx, z, len(z), 256, e2, 2, C.byref(info2), u64([0] * 3)) == BZX_E_PARAM


@pytest.mark.gpu
def test_gpu_count_records_call_order(gpu16, crafted):
    raw, z, e, n, table, pos = crafted
    L = gpu16.lib
    h = C.c_void_p()
    assert L.bzx_salvage_begin(gpu16.ctx, 0, C.byref(h)) == 0
    try:
        assert L.bzx_index_count_records(h, 10) == BZX_E_STATE
    finally:
        L.bzx_index_end(h)
    assert L.bzx_index_begin(gpu16.ctx, 0, C.byref(h)) == 0
    try:
        assert L.bzx_index_count_records(h, 256) == BZX_E_PARAM and L.bzx_index_count_records(h, -1) == BZX_E_PARAM
        used, done = C.c_size_t(), C.c_int()
        buf = C.create_string_buffer(z[:100], 100)
        assert L.bzx_index_feed(h, C.addressof(buf), 100, 0, C.byref(used), C.byref(done)) == 0
        assert L.bzx_index_count_records(h, 10) == BZX_E_STATE
    finally:
        L.bzx_index_end(h)


@pytest.mark.gpu
def test_gpu_table_from_the_raw_side(gpu16):
    from bzx_cindex_ctypes import CIndexLib
    maker = CIndexLib(max_blocks=16)
    try:
        raw = bytearray(RC.letters(1_300_000, 8)) + bytes(5000) + bytearray(RC.letters(40_000, 9))
        rnd = random.Random(12)
        for _ in range(20_000):
            raw[rnd.randrange(len(raw))] = 10
        raw = bytes(raw)
        assert maker.keep_index(True) == 0
        rc, z = maker.compress_buffer_rc(raw, 3, len(raw) + len(raw) // 50 + 4096)
        assert rc == 0 and bz2.decompress(z) == raw
        ep, info = C.POINTER(IndexEntry)(), IndexInfo()
        assert maker.lib.bzx_compress_get_index(maker.ctx, C.byref(ep), C.byref(info)) == 0
        n = info.nblk
        kept = (IndexEntry * n).from_buffer_copy(C.string_at(ep, 40 * n))
        rc, t_raw = gpu16.records_count_buffer(raw, 10, kept, n)
        assert rc == 0, gpu16.last_error()
        rc, e, info2, t_ix = gpu16.index_records(z, 10)
        assert rc == 0 and info2.nblk == n and t_raw == t_ix and n >= 4
        assert t_ix == RC.table_of(RC.positions(raw, 10), [e[k].out_off for k in range(n)])
        # entries that do not tile [0, len)
        assert gpu16.records_count_buffer(raw[:-1], 10, kept, n)[0] == BZX_E_PARAM
        kept[1].out_off += 1
        assert gpu16.records_count_buffer(raw, 10, kept, n)[0] == BZX_E_PARAM
    finally:
        maker.close()


@pytest.mark.gpu
def test_gpu_damaged_block(gpu16, crafted):
    raw, z, e, n, table, pos = crafted
    bad = bytearray(z)
    bad[(e[2].bit + e[2].img_bits // 2) // 8] ^= 0x10
    bad = bytes(bad)
    rc, e2, info2, t2 = gpu16.index_records(bad, 10)
    assert rc == BZX_E_DATA and info2.nblk == 2 and t2 == table[:3]
    T = len(pos)
    ranges = [(0, 2), (T - 1, 1), (T, 1), (table[1], 3), (T - 1, 2), (5, 5), (0, T + 1)]
    want = want_records(raw, pos, ranges)
    r = gpu16.records_buffer(bad, None, e, n, table, 10, ranges, sum(map(len, want)))
    touches = [False, False, True, False, True, False, True]      # record T starts on the first byte of block 2
    assert r.rc == BZX_E_DATA and r.status == [BZX_E_DATA if t else 0 for t in touches], gpu16.last_error()
    assert gpu16.last_error().startswith("range 2: ")
    for i, w in enumerate(want):
        assert r.gots[i] == (0 if touches[i] else len(w)) and (touches[i] or r.data(i) == w)


@pytest.mark.gpu
def test_gpu_stale_table(gpu16, crafted):
    raw, z, e, n, table, pos = crafted
    stale = list(table)
    stale[2] -= 1                                                       # one count moved from block 1 to block 2
    recs = [1, 5, table[1], table[1] + 1, table[1] + 2]
    rc, offs, st = gpu16.locate_buffer(z, None, e, n, stale, 10, recs)
    assert rc == BZX_E_DATA and st == [0, 0, 0, BZX_E_DATA, BZX_E_DATA]
    text = gpu16.last_error()
    assert text.startswith("query 3: record table does not match the input: block 1 holds ") and "the table says" in text
    assert offs[:3] == [RC.rec_start(pos, len(raw), r) for r in recs[:3]]
