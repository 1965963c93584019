"""Batched range reads (bzx_index_spans, bzx_decompress_ranges_*) and the gather kernel behind them (bzx_stage_gather).

The rules: range i of a call leaves what bzx_decompress_range_buffer leaves for that range alone
(bz2.decompress(z)[off:off + want]) at out_offs[i], the running sum of the clipped lengths; every distinct touched block
is decoded once; a damaged block or a stale entry fails exactly the ranges that touch it; the pieces bzx_index_spans
names are enough; the gather kernel copies any slice to any place, whatever the two alignments.
CPU part (-m "not gpu"): everything through the fiber emulator (tests/emu), small inputs.
GPU part (-m gpu): the product library on cuda:0."""
import bz2
import ctypes as C
import os
import random
import subprocess

import pytest

import bz2_writer as W
from bzx_ctypes import EMU_PATH, ROOT
from bzx_ranges_ctypes import RangesLib, u64
from test_range import build, few, index_inputs, range_plan, stale, text

BZX_OK, BZX_E_PARAM, BZX_E_OUTBUF, BZX_E_STATE, BZX_E_DATA = 0, -2, -4, -6, -7
PIECE = 64 << 10                                  # bytes of one entry of the gather kernel's table
EDGE = (900_000 // 5 * 259 + 16 + 255) & ~255     # one of the two staging areas that make the pool


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = RangesLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


# ---- 1. the gather kernel alone ---------------------------------------------------------------------------------------
LENGTHS = (0, 1, 15, 16, 17, 31, 33, 255, 256, 257, 4095, 4097, 65535, 65536, 65537, 200_001)
ALL_PAIRS = [(s, d) for s in range(16) for d in range(16)]
FEW_PAIRS = [(0, 0), (0, 1), (1, 0), (15, 15), (4, 0), (0, 4), (3, 7), (8, 8), (5, 13), (12, 2), (7, 7), (15, 0), (0, 15),
             (2, 6), (9, 10), (13, 3), (6, 11)]


def gather_case(lib, rnd, length, pairs):
    """One call: one slice of `length` bytes per (source alignment, destination alignment) pair, each into a region of
    its own of a 0xA5-filled output."""
    src = rnd.randbytes(length + 4096)
    stride = (length + 48 + 15) & ~15
    slices = []
    for i, (s, d) in enumerate(pairs):
        slices.append((16 * rnd.randrange(0, 255) + s, i * stride + 16 + d, length))
    out = b"\xa5" * (stride * len(pairs))
    rc, got = lib.stage_gather(src, slices, out)
    assert rc == 0, lib.last_error()
    exp = bytearray(out)
    for so, do, ln in slices:
        exp[do:do + ln] = src[so:so + ln]
    if got != bytes(exp):
        for (s, d), (so, do, ln) in zip(pairs, slices):
            assert got[do - 16 - d:do - 16 - d + stride] == bytes(exp[do - 16 - d:do - 16 - d + stride]), (length, s, d)
    assert got == bytes(exp)


def gather_grid(lib):
    rnd = random.Random(5)
    for length in LENGTHS:
        gather_case(lib, rnd, length, ALL_PAIRS if length in (1, 17, 65537) else FEW_PAIRS)
    # 300 slices of seeded offsets and lengths in one call, some reading the same source bytes; destinations packed
    src = rnd.randbytes(300_000)
    slices, at = [], 3
    for i in range(300):
        ln = rnd.choice((0, 1, 7, 100, 4096, 70_000, rnd.randrange(0, 20_000)))
        so = rnd.randrange(0, 1000) if i % 3 == 0 else rnd.randrange(0, len(src) - ln)      # (every third: overlapping)
        slices.append((so, at, ln))
        at += ln
    out = b"\xa5" * (at + 5)
    rc, got = lib.stage_gather(src, slices, out)
    assert rc == 0, lib.last_error()
    assert got == b"\xa5" * 3 + b"".join(src[so:so + ln] for so, _, ln in slices) + b"\xa5" * 5
    # a slice that leaves a buffer
    for bad in ((len(src) - 4, 0, 5), (0, len(out) - 4, 5), (len(src) + 1, 0, 0), (0, 0, 1 << 63)):
        rc, got = lib.stage_gather(src, [(0, 0, 4), bad], out)
        assert rc == BZX_E_PARAM and got == out, bad
    rc, got = lib.stage_gather(src, [], out)
    assert rc == 0 and got == out


def test_emu_gather(emu):
    gather_grid(emu)


# ---- 2. parity with the single call -------------------------------------------------------------------------------------
def touched(lib, entries, n, ranges):
    """The distinct blocks a list of ranges touches."""
    out = set()
    for off, w in ranges:
        rc, first, count, _, _ = lib.span(entries, n, off, w)
        assert rc == 0
        out |= set(range(first, first + count))
    return out


def py_spans(entries, blocks):
    """The union of the blocks' byte intervals, overlapping or adjacent ones merged."""
    out = []
    for k in sorted(blocks):
        lo, hi = entries[k].bit // 8, (entries[k].bit + entries[k].img_bits + 7) // 8 + 8
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi - lo) for lo, hi in out]


def check_call(lib, z, want, entries, n, ranges, how):
    """One _buffer call over `ranges`, with the whole file as one piece or with the pieces of bzx_index_spans."""
    pieces = None
    if how == "spans":
        rc, pieces, np = lib.spans(entries, n, ranges)
        assert rc == 0 and np == len(pieces)
        blocks = touched(lib, entries, n, ranges)
        assert pieces == py_spans(entries, blocks)                                  # the exact union
        assert all(a[0] + a[1] < b[0] for a, b in zip(pieces, pieces[1:]))          # ascending, disjoint, not adjacent
        assert all(b in {entries[k].bit // 8 for k in blocks} for b, _ in pieces)
    r = lib.ranges_buffer(z, pieces, entries, n, ranges)
    assert r.rc == 0, (how, len(ranges), lib.last_error())
    at = 0
    for i, (off, w) in enumerate(ranges):
        exp = want[off:off + w]
        assert r.out_offs[i] == at and r.gots[i] == len(exp) and r.status[i] == 0, (i, off, w)
        assert r.data(i) == exp, (i, off, w, how)
        at += len(exp)
    assert r.need == at
    if ranges:
        st = lib.stats()
        assert st.nblk == len(touched(lib, entries, n, ranges)) and st.raw_bytes == at
    return r


def parity_lists(entries, n, total, rnd, count=200):
    plan = range_plan(entries, n, total, rnd, count)
    rand = [(rnd.randrange(0, total + 2), rnd.choice((1, 2, 9, 40, 100, total))) for _ in range(200)]
    rnd.shuffle(rand)
    return [[], [plan[len(plan) // 2]], plan, rand, [r for r in plan[::3] for _ in (0, 1)]]


def many_blocks(oracle):
    """The 37-block stream of test_emu_range_rounds."""
    return W.write_stream(oracle, [W.Block(few(oracle, 12 + k % 5, 100 + k % 4, b"ab")) for k in range(37)], 9)


def parity(lib, oracle, seed):
    rnd = random.Random(seed)
    inputs = [(name, z) for name, z, _, _ in index_inputs(oracle)] + [("37 blocks", many_blocks(oracle))]
    for name, z in inputs:
        want = bz2.decompress(z)
        entries, n, _ = build(lib, z)
        for ranges in parity_lists(entries, n, len(want), rnd):
            for how in ("file", "spans"):
                check_call(lib, z, want, entries, n, ranges, how)


def test_emu_ranges_parity(emu, oracle):
    parity(emu, oracle, 29)


def test_emu_ranges_dedup_and_rounds(emu, oracle):
    z = many_blocks(oracle)
    want = bz2.decompress(z)
    entries, n, _ = build(emu, z)
    assert n == 37
    rnd = random.Random(31)
    # 50 ranges inside one block: one block decoded
    e = entries[5]
    ranges = [(e.out_off + rnd.randrange(0, e.out_len), rnd.randrange(0, 4)) for _ in range(50)]
    ranges = [(o, min(w, e.out_off + e.out_len - o)) for o, w in ranges]
    check_call(emu, z, want, entries, n, ranges, "spans")
    assert emu.stats().nblk == 1
    # more distinct blocks than two rounds of a 16-slab context hold; every other block, so the pieces have gaps too
    for step in (1, 2):
        ranges = [(entries[k].out_off + 1, 3) for k in range(0, 37, step)]
        rnd.shuffle(ranges)
        check_call(emu, z, want, entries, n, ranges, "spans")
        assert emu.stats().nblk == len(range(0, 37, step)) and (step == 2 or emu.stats().nblk > 32)
    # a block wholly inside one range that a second, small range touches as well: it goes through the pool
    a = (entries[3].out_off - 2, entries[6].out_off - entries[3].out_off + 4)
    b = (entries[4].out_off + 2, 5)
    for ranges in ([a, b], [b, a], [a, a], [a]):
        check_call(emu, z, want, entries, n, ranges, "file")
        assert emu.stats().nblk == 5


def test_emu_index_spans(emu, oracle):
    z = many_blocks(oracle)
    want = bz2.decompress(z)
    entries, n, _ = build(emu, z)
    ranges = [(entries[k].out_off + 1, 3) for k in (30, 2, 3, 9, 20, 21, 22)] + [(len(want) + 5, 9), (4, 0)]
    rc, pieces, np = emu.spans(entries, n, ranges)
    assert rc == 0 and np == len(pieces) and pieces == py_spans(entries, {2, 3, 9, 20, 21, 22, 30}) and 3 <= np <= 4
    assert emu.spans(entries, n, [])[::2] == (0, 0) and emu.spans(entries, n, [(len(want), 4)])[::2] == (0, 0)
    # too few pieces: the number needed
    rc, first, need = emu.spans(entries, n, ranges, cap=np - 1)
    assert rc == BZX_E_OUTBUF and need == np and first == pieces[:np - 1]
    # the last byte of one piece dropped: the whole call is refused, nothing is written
    for k in range(np):
        short = [(b, ln - (i == k)) for i, (b, ln) in enumerate(pieces)]
        r = emu.ranges_buffer(z, short, entries, n, ranges)
        assert r.rc == BZX_E_PARAM and r.room == b"\xa5" * len(r.room) and r.status == [BZX_E_PARAM] * len(ranges)
        assert r.gots == [0] * len(ranges) and "range " in emu.last_error() and "do not cover bytes [" in emu.last_error()
    # pieces that are not ascending and disjoint
    r = emu.ranges_buffer(z, [pieces[1], pieces[0]] + pieces[2:], entries, n, ranges)
    assert r.rc == BZX_E_PARAM and r.status == [BZX_E_PARAM] * len(ranges)
    r = emu.ranges_buffer(z, [(0, len(z)), (len(z) - 1, 1)], entries, n, ranges)
    assert r.rc == BZX_E_PARAM
    # entries that are not in output order
    rc, _, _ = emu.spans(stale(entries, n, 4, out_off=entries[9].out_off), n, [(entries[4].out_off, 3)])
    assert rc == BZX_E_PARAM
    r = emu.ranges_buffer(z, None, stale(entries, n, 4, out_off=entries[9].out_off), n, [(entries[4].out_off, 3)], cap=3)
    assert r.rc == BZX_E_PARAM and r.status == [BZX_E_PARAM]
    # a superset is accepted
    check_call(emu, z, want, entries, n, ranges, "spans")
    r = emu.ranges_buffer(z, [(pieces[0][0], pieces[-1][0] + pieces[-1][1] - pieces[0][0])], entries, n, ranges)
    assert r.rc == 0 and [r.data(i) for i in range(len(ranges))] == [want[o:o + w] for o, w in ranges]


# ---- 3. independence and refusals ---------------------------------------------------------------------------------------
def three_blocks(oracle):
    """The 3-block stream of test_emu_range_refusals -> (z, the same with a payload bit of block 2 flipped)."""
    b = [W.Block(few(oracle, 70, 21)), W.Block(few(oracle, 60, 22, b"klmno")), W.Block(few(oracle, 50, 23))]
    f = {}
    z = W.write_stream(oracle, b, 1, fields=f)
    bit = f["payload"][1][0] + (f["payload"][1][1] - f["payload"][1][0]) // 2
    bad = bytearray(z)
    bad[bit >> 3] ^= 0x80 >> (bit & 7)
    return z, bytes(bad)


def check_independent(lib, z, want, entries, true_entries, n, ranges, bad_block, text_part):
    """Exactly the ranges that touch bad_block fail; the others carry their bytes."""
    hit = [bad_block in touched(lib, true_entries, n, [r]) for r in ranges]
    assert any(hit) and not all(hit) and not hit[0]
    r = lib.ranges_buffer(z, None, entries, n, ranges, cap=sum(len(want[o:o + w]) for o, w in ranges))
    k = hit.index(True)
    assert r.rc == BZX_E_DATA == r.status[k], (r.rc, r.status, lib.last_error())
    msg = lib.last_error()
    assert msg.startswith(f"range {k}: ") and (text_part is None or text_part in msg), msg
    at = 0
    for i, (off, w) in enumerate(ranges):
        exp = want[off:off + w]
        assert r.out_offs[i] == at
        if hit[i]:
            assert r.status[i] == BZX_E_DATA and r.gots[i] == 0 and r.room[at:at + len(exp)] == b"\xa5" * len(exp), i
        else:
            assert r.status[i] == 0 and r.data(i) == exp, (i, off, w)
        at += len(exp)
    assert r.need == at
    return msg


def test_emu_ranges_independence(emu, oracle):
    z, bad = three_blocks(oracle)
    want = bz2.decompress(z)
    entries, n, _ = build(emu, z)
    e = entries
    ranges = [(e[0].out_off + 3, 9), (e[2].out_off + 4, 11), (e[1].out_off + 5, 20), (e[0].out_off + 40, 50), (e[2].out_off + 1, 1),
              (e[1].out_off + 10, 1), (e[0].out_off + 1, 2), (e[1].out_off + 30, 60), (e[2].out_off + 20, 100), (0, len(want))]
    msg = check_independent(emu, bad, want, entries, entries, n, ranges, 1, None)
    assert "index does not match the input" in msg or "block CRC mismatch in block 1" in msg or "damaged block" in msg
    for name, change in (("crc", {"crc": e[1].crc ^ 4}), ("out_len", {"out_len": e[1].out_len - 1}), ("bit", {"bit": e[1].bit + 1})):
        check_independent(emu, z, want, stale(entries, n, 1, **change), entries, n, ranges[:-1], 1, "index does not match the input")
        # after that a clean call on the same context succeeds
        check_call(emu, z, want, entries, n, ranges, "file")
    # the whole list fails: the lowest range is named
    r = emu.ranges_buffer(bad, None, entries, n, [(e[1].out_off, 4), (e[1].out_off + 9, 4)])
    assert r.rc == BZX_E_DATA and r.status == [BZX_E_DATA] * 2 and emu.last_error().startswith("range 0: ") and r.room == b"\xa5" * 8


def test_emu_ranges_refusals(emu, oracle):
    z, _ = three_blocks(oracle)
    want = bz2.decompress(z)
    entries, n, _ = build(emu, z)
    ranges = [(entries[1].out_off + 5, 20), (3, 0), (len(want) - 4, 50), (0, 100), (len(want) + 1, 5)]
    need = sum(len(want[o:o + w]) for o, w in ranges)
    # one byte short
    r = emu.ranges_buffer(z, None, entries, n, ranges, cap=need - 1)
    assert r.rc == BZX_E_OUTBUF and r.need == need and r.room == b"\xa5" * (need - 1) and r.status == [BZX_E_OUTBUF] * len(ranges)
    r = check_call(emu, z, want, entries, n, ranges, "file")
    assert r.need == need
    # an open bzx_dstream
    s = emu.dstream(64)
    try:
        r = emu.ranges_buffer(z, None, entries, n, ranges)
        assert r.rc == BZX_E_STATE and r.status == [BZX_E_STATE] * len(ranges) and "bzx_dstream" in emu.last_error()
        assert r.room == b"\xa5" * need
        assert emu.stage_gather(b"abc", [(0, 0, 1)], b"xyz")[0] == BZX_E_STATE
    finally:
        s.end()
    # ... and an open index
    h = C.c_void_p()
    assert emu.lib.bzx_index_begin(emu.ctx, 0, C.byref(h)) == 0
    try:
        assert emu.ranges_buffer(z, None, entries, n, ranges).rc == BZX_E_STATE
    finally:
        emu.lib.bzx_index_end(h)
    check_call(emu, z, want, entries, n, ranges, "spans")
    # NULL arguments
    L = emu.lib
    fn = L.bzx_decompress_ranges_buffer
    zb = C.create_string_buffer(z, len(z))
    from bzx_ranges_ctypes import Piece
    pc = (Piece * 1)(Piece(C.addressof(zb), 0, len(z)))
    offs, wants = u64([0, 7]), u64([5, 5])
    so, sg, st, nd = (C.c_size_t * 2)(), (C.c_size_t * 2)(), (C.c_int * 2)(), C.c_size_t()
    out = C.create_string_buffer(10)
    good = [emu.ctx, pc, 1, entries, n, 2, offs, wants, C.addressof(out), 10, so, sg, st, C.byref(nd)]
    assert fn(*good) == 0 and out.raw == want[0:5] + want[7:12]
    for k in (0, 1, 3, 6, 7, 8, 10, 11, 12, 13):
        args = list(good)
        args[k] = None
        st[0] = st[1] = 77
        assert fn(*args) == BZX_E_PARAM, k
        assert k in (0, 12) or list(st) == [BZX_E_PARAM] * 2, k
    args = list(good)
    args[5] = 0                                                               # count 0: nothing is looked at
    for k in (1, 3, 6, 7, 8, 10, 11, 12):
        args[k] = None
    assert fn(*args) == 0
    assert L.bzx_index_spans(entries, n, 1, offs, wants, None, None, 0, None) == BZX_E_PARAM
    assert L.bzx_index_spans(entries, n, 1, None, wants, offs, wants, 1, C.byref(C.c_uint32())) == BZX_E_PARAM
    assert L.bzx_index_spans(entries, n, 1, offs, wants, None, None, 1, C.byref(C.c_uint32())) == BZX_E_PARAM
    assert fn(*good) == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu16():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = RangesLib(max_blocks=16)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def maker():
    """A context of its own for making the inputs (compression grows a context's slabs)."""
    lib = RangesLib(max_blocks=16)
    yield lib
    lib.close()


def device_call(lib, z, entries, n, ranges, need, shift=1):
    """Through bzx_decompress_ranges_device: the whole file on the device at an odd address, d_out at an odd address, a
    guard byte behind *need -> (RangesResult, the output bytes, the guard byte)"""
    import torch
    d_z = torch.empty(len(z) + 16, dtype=torch.uint8, device="cuda")
    d_z[3:3 + len(z)] = torch.frombuffer(bytearray(z), dtype=torch.uint8).cuda()
    d_o = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = lib.ranges_raw(lib.lib.bzx_decompress_ranges_device, [(d_z.data_ptr() + 3, 0, len(z))], entries, n, ranges,
                       d_o.data_ptr() + shift, need)
    torch.cuda.synchronize()
    back = d_o.cpu().numpy().tobytes()
    r.room = back[shift:shift + need]
    return r, back[shift + need], back[:shift]


@pytest.mark.gpu
def test_gpu_gather(gpu16):
    gather_grid(gpu16)


@pytest.mark.gpu
def test_gpu_ranges_small_shapes(gpu16, oracle):
    parity(gpu16, oracle, 37)


@pytest.mark.gpu
def test_gpu_ranges_text(gpu16, maker, oracle):
    rnd = random.Random(53)
    raw = text(oracle, 8 << 20, 83)
    z = maker.compress_buffer(raw, 1)
    rc, entries, info = gpu16.index_build(z, cap=4096)
    n = info.nblk
    assert rc == 0 and n >= 80 and info.out_bytes == len(raw)
    ranges = []
    for k in rnd.sample(range(1, n), 6):                                       # the block borders
        for d in (-2, -1, 0, 1):
            ranges += [(entries[k].out_off + d, 1), (entries[k].out_off + d, 3), (entries[k].out_off + d - 2, 70_000)]
    ranges += [(0, 0), (len(raw), 5), (len(raw) + 1, 5), (len(raw) - 1, 9), (0, 1)]
    for _ in range(500):
        w = 1 << rnd.randrange(0, 18)
        ranges.append((rnd.randrange(0, len(raw)), min(256 << 10, rnd.randrange(w, 2 * w + 1))))
    rnd.shuffle(ranges)
    blocks = touched(gpu16, entries, n, ranges)
    check_call(gpu16, z, raw, entries, n, ranges, "spans")
    assert gpu16.stats().nblk == len(blocks) > 16
    need = sum(len(raw[o:o + w]) for o, w in ranges)
    r, guard, front = device_call(gpu16, z, entries, n, ranges, need)
    assert r.rc == 0 and r.need == need and guard == 0xA5 and front == b"\xa5", gpu16.last_error()
    assert r.status == [0] * len(ranges) and all(r.data(i) == raw[o:o + w] for i, (o, w) in enumerate(ranges))
    assert gpu16.stats().nblk == len(blocks) and gpu16.stats().raw_bytes == need
    s = gpu16.dstream(1 << 20)                                   # the range reads left the slabs alone
    assert s.info().slabs == 16
    s.end()


@pytest.mark.gpu
def test_gpu_ranges_pool_rule(gpu16, maker):
    total = 128 << 20
    z = maker.compress_buffer(bytes(total), 9)
    assert len(z) < 1000
    rc, entries, info = gpu16.index_build(z)
    assert rc == 0 and info.nblk == 3 and info.out_bytes == total
    n = 3
    al = [(entries[k].out_len + 255) & ~255 for k in range(n)]
    assert al[0] + al[1] <= 2 * EDGE < al[0] + al[1] + al[2]                  # two pool blocks fit, the third does not: two rounds
    rnd = random.Random(59)
    ranges = [(rnd.randrange(entries[k].out_off, entries[k].out_off + entries[k].out_len - (1 << 20)), rnd.randrange(1, 1 << 20))
              for k in (0, 1, 2) for _ in range(6)]
    ranges += [(entries[1].out_off - 70_001, 140_003), (entries[2].out_off - 1, 2)]          # across the two borders
    rnd.shuffle(ranges)
    assert len(ranges) == 20 and touched(gpu16, entries, n, ranges) == {0, 1, 2}
    need = sum(w for _, w in ranges)
    r, guard, front = device_call(gpu16, z, entries, n, ranges, need, shift=3)
    assert r.rc == 0 and r.need == need and guard == 0xA5 and front == b"\xa5" * 3, gpu16.last_error()
    assert r.gots == [w for _, w in ranges] and r.status == [0] * 20 and r.room == bytes(need)
    assert gpu16.stats().nblk == 3
    rc, pieces, np = gpu16.spans(entries, n, ranges)
    r = gpu16.ranges_buffer(z, pieces, entries, n, ranges)
    assert r.rc == 0 and r.room == bytes(need)


@pytest.mark.gpu
def test_gpu_ranges_damage(gpu16, maker, oracle):
    raw = text(oracle, 3 << 20, 95)
    z = maker.compress_buffer(raw, 1)
    rc, entries, info = gpu16.index_build(z)
    n = info.nblk
    assert rc == 0 and n >= 30
    bad = bytearray(z)
    bad[(entries[10].bit + entries[10].img_bits // 2) // 8] ^= 0x10
    e = entries
    ranges = [(e[9].out_off + 1000, 5000), (e[10].out_off + 1000, 5000), (e[11].out_off, 70_000), (e[11].out_off - 100, 300),
              (e[9].out_off, e[9].out_len), (e[10].out_off, e[10].out_len), (e[10].out_off - 1, 1), (e[12].out_off + 5, 200_000)]
    check_independent(gpu16, bytes(bad), raw, entries, entries, n, ranges, 10, None)
    check_independent(gpu16, z, raw, stale(entries, n, 10, crc=1), entries, n, ranges, 10, "index does not match the input")
    check_call(gpu16, z, raw, entries, n, ranges, "spans")
