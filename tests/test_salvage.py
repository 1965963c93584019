"""Salvage (bzx_salvage_*): the index of every intact block of a damaged .bz2, and the gaps between them.

The rule is in include/bzx.h.  Expectations come from the writer's map of bit fields (tests/bz2_writer.py), from the
blocks' raw() and from bz2, never from the library under test: a surviving block's entry is (bit of its magic, re-summed
out_off, len(raw), CRC of raw, bits from its magic to its last payload bit, markers passed, level of the walk).
CPU part (-m "not gpu"): everything through the fiber emulator (tests/emu), blocks of 40..80 bytes.
GPU part (-m gpu): the product library on cuda:0."""
import bz2
import ctypes as C
import os
import random
import subprocess

import pytest

import bz2_writer as W
from bzx_ctypes import EMU_PATH, ROOT
from bzx_salvage_ctypes import (GAP_BLOCK_CRC, GAP_COMBINED_CRC, GAP_HEADER, GAP_NO_MAGIC, GAP_RANDOMISED, GAP_STRUCTURE,
                                GAP_TRUNCATED, Gap, SalvageLib)
from test_range import few, index_inputs, text

BZX_OK, BZX_E_PARAM, BZX_E_OUTBUF = 0, -2, -4
CUTS = [(feeds, mc) for feeds in (1, 7, 4096, 0) for mc in ((16, 64, 1 << 16) if feeds == 7 else (64,) if feeds == 1 else (256, 0))]


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = SalvageLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


# ---- damage ---------------------------------------------------------------------------------------------------------------
def flip(z, bit):
    z = bytearray(z)
    z[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(z)


def zero_bits(z, lo, hi):
    z = bytearray(z)
    for bit in range(lo, hi):
        z[bit >> 3] &= ~(0x80 >> (bit & 7)) & 0xFF
    return bytes(z)


def mid(f, name, k):
    lo, hi = f[name][k]
    return lo + (hi - lo) // 2


class Stream:
    """One written stream: its bytes, the bit fields of its parts and what a clean walk makes of its blocks."""

    def __init__(self, o, blocks, level, **kw):
        self.o, self.blocks, self.level, self.f = o, blocks, level, {}
        self.z = W.write_stream(o, blocks, level, fields=self.f, **kw)
        self.magic = [s for s, _ in self.f["magic"]]
        self.eos = self.f["eos"][0][0]

    def keys(self, alive, base_bit=0, out_off=0, stream=0, level=None):
        """Entry keys of the blocks `alive`, the output re-summed from out_off."""
        out = []
        for i in alive:
            raw = self.blocks[i].raw()
            out.append((base_bit + self.magic[i], out_off, len(raw), self.o.crc32(raw), self.f["payload"][i][1] - self.magic[i],
                        stream, self.level if level is None else level))
            out_off += len(raw)
        return out

    def raw(self, alive):
        return b"".join(self.blocks[i].raw() for i in alive)


def four(o):
    return [W.Block(few(o, 70, 21)), W.Block(few(o, 60, 22, b"klmno")), W.Block(few(o, 50, 23)), W.Block(few(o, 55, 24, b"xyz"))]


def reason_cases(o):
    """(name, input, entry keys, surviving bytes, [(bit_lo, bit_hi, out_off, candidates, why it must name, why it may name)])"""
    s = Stream(o, four(o), 1)
    z, m, n = s.z, s.magic, [len(b.raw()) for b in s.blocks]
    total = sum(n)
    out = []

    def case(name, bad, alive, gaps, st=s, **kw):
        out.append((name, bad, st.keys(alive, **kw), st.raw(alive), [g if len(g) == 6 else g + (g[4],) for g in gaps]))
    case("stored CRC of block 2 flipped", flip(z, mid(s.f, "crc", 1)), [0, 2, 3], [(m[1], m[2], n[0], 1, GAP_BLOCK_CRC)])
    case("magic of block 2 zeroed", zero_bits(z, m[1], m[1] + 48), [0, 2, 3], [(m[1], m[2], n[0], 0, GAP_NO_MAGIC)])
    b = four(o)
    b[1] = W.Block(b[1].image, randomised=1)
    r = Stream(o, b, 1)
    case("a randomised block", r.z, [0, 2, 3], [(r.magic[1], r.magic[2], n[0], 1, GAP_RANDOMISED)], st=r)
    b = four(o)
    b[1] = W.Block(b"a" * 100001)
    r = Stream(o, b, 1)
    case("a block longer than its level allows", r.z, [0, 2, 3], [(r.magic[1], r.magic[2], n[0], 1, GAP_STRUCTURE)], st=r)
    case("blocks 2 and 3 both hit", flip(flip(z, mid(s.f, "crc", 1)), mid(s.f, "payload", 2)), [0, 3],
         [(m[1], m[3], n[0], 2, GAP_BLOCK_CRC, GAP_BLOCK_CRC | GAP_STRUCTURE)])
    cut = z[:s.f["payload"][2][0] // 8 + 3]
    case("truncated inside block 3", cut, [0, 1], [(m[2], 8 * len(cut), n[0] + n[1], 1, GAP_STRUCTURE | GAP_TRUNCATED)])
    # ... exactly before the end-of-stream marker: a last block that ends on a byte boundary
    for k in range(40, 81):
        b = four(o)[:3] + [W.Block(few(o, k, 24, b"xyz"))]
        r = Stream(o, b, 1)
        if r.eos % 8 == 0:
            break
    assert r.eos % 8 == 0
    case("truncated exactly before the end-of-stream marker", r.z[:r.eos // 8], [0, 1, 2, 3],
         [(r.eos, r.eos, len(r.raw(range(4))), 0, GAP_TRUNCATED)], st=r)
    good = W.stream_crc([o.crc32(x.raw()) for x in s.blocks])
    r = Stream(o, four(o), 1, combined_crc=good ^ 0x10)
    case("combined CRC wrong", r.z, [0, 1, 2, 3], [(r.eos, r.eos, total, 0, GAP_COMBINED_CRC)], st=r)
    case("bytes 0..3 zeroed", bytes(4) + z[4:], [0, 1, 2, 3], [(0, 32, 0, 0, GAP_HEADER)], level=9)
    return out


def stream_cases(o):
    a = Stream(o, [W.Block(few(o, 60, 41)), W.Block(few(o, 45, 42, b"xyz"))], 2)
    b = Stream(o, [W.Block(few(o, 50, 43)), W.Block(few(o, 40, 44, b"pqrs"))], 5)
    c = Stream(o, [W.Block(few(o, 55, 45)), W.Block(few(o, 48, 46, b"uvw"))], 3)
    za, zb, zc = a.z, b"\0\0\0\0" + b.z[4:], flip(c.z, mid(c.f, "crc", 1))
    la, lb = 8 * len(za), 8 * (len(za) + len(zb))
    na, nb = len(a.raw([0, 1])), len(b.raw([0, 1]))
    keys = a.keys([0, 1]) + b.keys([0, 1], la, na, 1, 9) + c.keys([0], lb, na + nb, 2)
    gaps = [(la, la + 32, na, 0, GAP_NO_MAGIC | GAP_HEADER), (lb + c.magic[1], lb + c.eos, na + nb + len(c.raw([0])), 1, GAP_BLOCK_CRC)]
    return [("three streams, the middle header destroyed, the last block damaged", za + zb + zc, keys,
             a.raw([0, 1]) + b.raw([0, 1]) + c.raw([0]), [g + (g[4],) for g in gaps])]


def rounds_case(o, hit_crc=(15, 16, 32, 33), hit_magic=(17,), nblocks=40):
    """Rounds of 16 slabs: the last block of the first round (index 15), the first two of the second (16, 17), the first
    two of the third (32, 33)."""
    s = Stream(o, [W.Block(few(o, 12 + k % 5, 100 + k % 4, b"ab")) for k in range(nblocks)], 9)
    z = s.z
    for k in hit_crc:
        z = flip(z, mid(s.f, "crc", k))
    for k in hit_magic:
        z = zero_bits(z, s.magic[k], s.magic[k] + 48)
    alive = [k for k in range(nblocks) if k not in hit_crc + hit_magic]
    n = [len(b.raw()) for b in s.blocks]
    m = s.magic
    gaps = [(m[15], m[18], sum(n[:15]), 2, GAP_BLOCK_CRC, GAP_BLOCK_CRC), (m[32], m[34], sum(n[:32]) - n[15] - n[16] - n[17], 2,
                                                                         GAP_BLOCK_CRC, GAP_BLOCK_CRC)]
    return ("40 blocks, 15..17, 32 and 33 hit", z, s.keys(alive), s.raw(alive), gaps)


def info_key(info):
    return (info.in_bytes, info.out_bytes, info.nblk, info.nstreams)


def check_case(lib, case, nstreams, cuts=()):
    """One input through bzx_salvage_build_buffer (and every cutting of `cuts` through feed): the entries and gaps
    expected.  -> (entries, nblk)"""
    name, z, keys, alive, gaps = case
    rc, entries, info, got_gaps, ng = lib.salvage_build(z)
    assert rc == 0, (name, lib.last_error())
    got = [entries[i].key() for i in range(info.nblk)]
    assert got == keys, (name, got, keys)
    assert info_key(info) == (len(z), len(alive), len(keys), nstreams), (name, info_key(info))
    assert ng == len(got_gaps) == len(gaps), (name, got_gaps)
    for g, (lo, hi, out_off, cand, must, may) in zip(got_gaps, gaps):
        assert g[:4] == (lo, hi, out_off, cand) and g[4] & must == must and g[4] & ~may == 0, (name, g, gaps)
    for feeds, max_chunk in cuts:
        rc, k2, inf2, g2 = lib.salvage_feed(z, feeds, max_chunk)
        assert rc == 0 and k2 == got and g2 == got_gaps and info_key(inf2) == info_key(info), (name, feeds, max_chunk, k2, g2)
    return entries, info.nblk


def padded(z, entries, n):
    """The range reader wants 8 bytes behind a block's image (bzx_index_span: byte_hi); a truncated input gets zeros."""
    if n and (entries[n - 1].bit + entries[n - 1].img_bits + 7) // 8 + 8 > len(z):
        return z + bytes(8)
    return z


def check_reading(lib, case, entries, n):
    name, z, keys, alive, gaps = case
    rc, got, _, _ = lib.range_buffer(padded(z, entries, n), 0, entries, n, 0, len(alive))
    assert rc == 0 and got == alive, (name, rc, lib.last_error())
    rc, got, out_len, g, ng = lib.salvage_buffer(z, len(alive) + 5)
    assert rc == 0 and got == alive and out_len == len(alive) and ng == len(g) == len(gaps), (name, rc, lib.last_error())


# ---- emulator -------------------------------------------------------------------------------------------------------------
def test_emu_salvage_clean(emu, oracle):
    for name, z, expect, nstreams in index_inputs(oracle):
        rc, entries, info = emu.index_build(z)
        assert rc == 0
        keys = [entries[i].key() for i in range(info.nblk)]
        assert [(k[0], k[2], k[3], k[5], k[6]) for k in keys] == expect        # (as test_range.py holds it against the writer)
        rc, e2, inf2, gaps, ng = emu.salvage_build(z)
        assert rc == 0 and [e2[i].key() for i in range(inf2.nblk)] == keys, name
        assert bytes(e2)[:40 * inf2.nblk] == bytes(entries)[:40 * info.nblk]
        assert info_key(inf2) == info_key(info) == (len(z), len(bz2.decompress(z)), len(expect), nstreams), name
        if "stray magic" in name:
            last = keys[-1]
            after = (last[0] + last[4] + 80 + 7) // 8 * 8                       # the byte boundary behind the footer
            assert ng == 1 and gaps[0][:4] == (after, 8 * len(z), info.out_bytes, 1), (name, gaps)
            assert not gaps[0][4] & GAP_TRUNCATED
        else:
            assert ng == 0 and gaps == [], (name, gaps)
        for feeds, max_chunk in CUTS:
            rc, k2, inf3, g2 = emu.salvage_feed(z, feeds, max_chunk)
            assert rc == 0 and k2 == keys and g2 == gaps and info_key(inf3) == info_key(info), (name, feeds, max_chunk)
    # inputs that hold nothing
    for z, gap in ((b"", (0, 0, 0, 0, GAP_HEADER | GAP_TRUNCATED)), (b"BZh", (0, 24, 0, 0, GAP_HEADER | GAP_TRUNCATED)),
                   (b"BZh9", (32, 32, 0, 0, GAP_TRUNCATED)), (bz2.compress(b""), None)):
        rc, _, info, gaps, ng = emu.salvage_build(z)
        assert rc == 0 and info_key(info) == (len(z), 0, 0, 1 if gap is None else 0), (z, info_key(info))
        assert gaps == ([] if gap is None else [gap]), (z, gaps)
        rc, got, out_len, _, _ = emu.salvage_buffer(z, 4)
        assert rc == 0 and got == b"" and out_len == 0


def every_bit_flips(o):
    s = Stream(o, four(o), 1)
    lo, hi = s.magic[1], s.magic[2]
    assert hi - lo == 363
    return s, list(range(lo, hi))


def test_emu_salvage_every_bit_of_one_block(emu, oracle):
    """Block 2 is lost for every flip, blocks 1, 3 and 4 never: payload and n_selectors flips send the failed block's reader
    across blocks 3 and 4, whose magics are tried all the same."""
    s, bits = every_bit_flips(oracle)
    n = [len(b.raw()) for b in s.blocks]
    keys = s.keys([0, 2, 3])
    # what the expectation rests on: libbz2 refuses 362 of the 363 flips, and the one it accepts is the randomised bit
    accepted = []
    for bit in bits:
        try:
            bz2.decompress(flip(s.z, bit))
            accepted.append(bit)
        except (OSError, ValueError, EOFError):
            pass
    assert accepted == [s.f["randomised"][1][0]]
    # (the emulator needs four minutes for all 363: every field's first and last bit and a seeded sample of 60)
    edges = {b for name, spans in s.f.items() if len(spans) == 4 for b in (spans[1][0], spans[1][1] - 1) if spans[1][1] > spans[1][0]}
    assert len(edges) >= 18 and edges <= set(bits)
    bits = sorted(edges | set(random.Random(5).sample(bits, 60)))
    for bit in bits:
        rc, entries, info, gaps, ng = emu.salvage_build(flip(s.z, bit))
        assert rc == 0
        assert [entries[i].key() for i in range(info.nblk)] == keys, bit
        in_magic = bit < s.magic[1] + 48
        assert ng == 1 and gaps[0][:4] == (s.magic[1], s.magic[2], n[0], 0 if in_magic else 1), (bit, gaps)
        assert gaps[0][4] == GAP_NO_MAGIC if in_magic else gaps[0][4] & (GAP_STRUCTURE | GAP_BLOCK_CRC | GAP_RANDOMISED)
        assert info_key(info) == (len(s.z), sum(n) - n[1], 3, 1)


def test_emu_salvage_reasons(emu, oracle):
    for case in reason_cases(oracle):
        cut = "truncated" in case[0]
        entries, n = check_case(emu, case, 0 if cut else 1, cuts=[(7, 16), (0, 0)])
        check_reading(emu, case, entries, n)


def test_emu_salvage_streams(emu, oracle):
    for case in stream_cases(oracle):
        entries, n = check_case(emu, case, 3, cuts=CUTS)
        assert [entries[i].stream for i in range(n)] == [0, 0, 1, 1, 2] and [entries[i].level for i in range(n)] == [2, 2, 9, 9, 3]
        check_reading(emu, case, entries, n)


def test_emu_salvage_cutting(emu, oracle):
    """Feeds of 7 bytes with max_chunk 16 and 64 cut through magics and through damaged blocks that are withheld."""
    cases = reason_cases(oracle)
    for case in (cases[0], cases[4], cases[5], cases[6]):
        check_case(emu, case, 0 if "truncated" in case[0] else 1, cuts=CUTS)
    # a flipped n_selectors bit: the reader of the failed block runs across every block behind it
    s = Stream(oracle, four(oracle), 1)
    n = [len(b.raw()) for b in s.blocks]
    for bit in (s.f["n_selectors"][1][0] + 1, mid(s.f, "payload", 1)):
        case = ("reader across blocks 3 and 4", flip(s.z, bit), s.keys([0, 2, 3]), s.raw([0, 2, 3]),
                [(s.magic[1], s.magic[2], n[0], 1, 0, GAP_STRUCTURE | GAP_BLOCK_CRC)])
        check_case(emu, case, 1, cuts=CUTS)


def test_emu_salvage_rounds(emu, oracle):
    """More candidates than the context holds slabs, damage at the borders of the rounds."""
    case = rounds_case(oracle)
    entries, n = check_case(emu, case, 1, cuts=[(7, 64), (0, 256)])
    assert n == 35
    check_reading(emu, case, entries, n)


def test_emu_salvage_reading_and_arguments(emu, oracle):
    case = reason_cases(oracle)[0]
    name, z, keys, alive, gaps = case
    # too little room: what is needed, and the first items
    rc, got, out_len, g, ng = emu.salvage_buffer(z, 100)
    assert rc == BZX_E_OUTBUF and out_len == len(alive) and got == alive[:100] and ng == 1
    rc, got, out_len, g, ng = emu.salvage_buffer(z, len(alive), cap_gaps=0)
    assert rc == BZX_E_OUTBUF and out_len == len(alive) and got == alive and (g, ng) == ([], 1)
    rc, entries, info, g, ng = emu.salvage_build(z, cap=2, cap_gaps=4)
    assert rc == BZX_E_OUTBUF and info.nblk == 3 and [entries[i].key() for i in range(2)] == keys[:2] and ng == 1
    rc, entries, info, g, ng = emu.salvage_build(z, cap_gaps=0)
    assert rc == BZX_E_OUTBUF and info.nblk == 3 and (g, ng) == ([], 1)
    # arguments, and a plain index has no gaps
    L = emu.lib
    h = C.c_void_p()
    assert L.bzx_salvage_begin(None, 0, C.byref(h)) == BZX_E_PARAM and L.bzx_salvage_begin(emu.ctx, 0, None) == BZX_E_PARAM
    assert L.bzx_salvage_buffer(emu.ctx, z, len(z), None, 5, C.byref(C.c_size_t()), None, 0, C.byref(C.c_uint64())) == BZX_E_PARAM
    assert L.bzx_index_begin(emu.ctx, 0, C.byref(h)) == 0
    try:
        gp, n = C.POINTER(Gap)(), C.c_uint64(7)
        assert L.bzx_index_get_gaps(h, C.byref(gp), C.byref(n)) == 0 and n.value == 0
        assert emu.salvage_build(z)[0] == -6                                     # BZX_E_STATE: the context is busy
    finally:
        L.bzx_index_end(h)
    # afterwards the context builds a clean index again
    s = Stream(oracle, four(oracle), 1)
    rc, entries, info = emu.index_build(s.z)
    assert rc == 0 and [entries[i].key() for i in range(info.nblk)] == s.keys(range(4))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu16():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = SalvageLib(max_blocks=16)
    yield lib
    lib.close()


def clean_index(lib, z, want):
    rc, entries, info = lib.index_build(z, cap=max(4096, len(z) // 2000))
    assert rc == 0 and info.out_bytes == len(want), lib.last_error()
    return entries, info.nblk, info


def salvaged(lib, z, cuts=((0, 0),)):
    """-> (entries, nblk, info, gaps): bzx_salvage_build_buffer, the same from every cutting."""
    rc, entries, info, gaps, ng = lib.salvage_build(z, cap=max(4096, len(z) // 2000))
    assert rc == 0 and ng == len(gaps), lib.last_error()
    keys = [entries[i].key() for i in range(info.nblk)]
    for feeds, max_chunk in cuts:
        rc, k2, inf2, g2 = lib.salvage_feed(z, feeds, max_chunk)
        assert rc == 0 and k2 == keys and g2 == gaps and info_key(inf2) == info_key(info), (feeds, max_chunk)
    return entries, info.nblk, info, gaps


def resummed(entries, alive, stream=None, level=None):
    out, off = [], 0
    for i in alive:
        k = entries[i].key()
        out.append((k[0], off, k[2], k[3], k[4], k[5] if stream is None else stream[i], k[6] if level is None else level[i]))
        off += k[2]
    return out


def pieces(entries, alive, want):
    return b"".join(want[entries[i].out_off:entries[i].out_off + entries[i].out_len] for i in alive)


@pytest.mark.gpu
def test_gpu_salvage_two_streams(gpu16, oracle):
    raw = [text(oracle, 450_000, 301), text(oracle, 450_000, 302)]
    z1, z2 = bz2.compress(raw[0], 1), bz2.compress(raw[1], 1)
    z, want = z1 + z2, raw[0] + raw[1]
    e, n, info = clean_index(gpu16, z, want)
    assert n == 10 and [e[i].stream for i in range(n)] == [0] * 5 + [1] * 5
    bad = flip(z, e[1].bit + e[1].img_bits // 2)                               # a payload bit of block 2
    bad = zero_bits(bad, e[3].bit, e[3].bit + 48)                              # the magic of block 4
    bad = bad[:len(z1)] + b"\0\0\0\0" + bad[len(z1) + 4:]                      # the second stream's header
    bad = bad[:(e[9].bit + e[9].img_bits // 2) // 8]                           # the end, inside the last block
    alive = [0, 2, 4, 5, 6, 7, 8]
    entries, nblk, inf, gaps = salvaged(gpu16, bad, cuts=((4096, 64 << 10),))
    assert [entries[i].key() for i in range(nblk)] == resummed(e, alive, level=[1] * 5 + [9] * 5)
    out = pieces(e, alive, want)
    assert info_key(inf) == (len(bad), len(out), 7, 1)
    off = [0, e[0].out_len, e[0].out_len + e[2].out_len, len(pieces(e, alive[:3], want)), len(out)]
    assert [g[:4] for g in gaps] == [(e[1].bit, e[2].bit, off[1], 1), (e[3].bit, e[4].bit, off[2], 0),
                                     (8 * len(z1), 8 * len(z1) + 32, off[3], 0), (e[9].bit, 8 * len(bad), off[4], 1)], gaps
    assert gaps[0][4] & (GAP_STRUCTURE | GAP_BLOCK_CRC) and gaps[1][4] == GAP_NO_MAGIC and gaps[2][4] == GAP_NO_MAGIC | GAP_HEADER
    assert gaps[3][4] == GAP_STRUCTURE | GAP_TRUNCATED
    rc, got, _, _ = gpu16.range_buffer(padded(bad, entries, nblk), 0, entries, nblk, 0, len(out))
    assert rc == 0 and got == out, gpu16.last_error()
    rc, got, out_len, g, ng = gpu16.salvage_buffer(bad, len(out))
    assert rc == 0 and got == out and out_len == len(out) and g == gaps
    rc, got, out_len, g, ng = gpu16.salvage_buffer(bad, 1000)
    assert rc == BZX_E_OUTBUF and out_len == len(out) and got == out[:1000]


@pytest.mark.gpu
def test_gpu_salvage_rounds(gpu16, oracle):
    """40 level-1 blocks on 16 slabs, damage at the borders of the rounds."""
    want = text(oracle, 40 * 99_000, 303)
    z = bz2.compress(want, 1)
    e, n, info = clean_index(gpu16, z, want)
    assert n == 40
    bad = z
    for k in (15, 16, 32):                                                     # blocks 16, 17 and 33
        bad = flip(bad, e[k].bit + e[k].img_bits // 2)
    alive = [k for k in range(40) if k not in (15, 16, 32)]
    entries, nblk, inf, gaps = salvaged(gpu16, bad, cuts=((1 << 20, 1 << 20),))
    assert [entries[i].key() for i in range(nblk)] == resummed(e, alive)
    out = pieces(e, alive, want)
    assert info_key(inf) == (len(z), len(out), 37, 1)
    assert [g[:4] for g in gaps] == [(e[15].bit, e[17].bit, e[15].out_off, 2),
                                     (e[32].bit, e[33].bit, e[32].out_off - e[15].out_len - e[16].out_len, 1)], gaps
    rc, got, out_len, _, _ = gpu16.salvage_buffer(bad, len(out))
    assert rc == 0 and got == out


@pytest.mark.gpu
def test_gpu_salvage_one_block_per_pass(gpu16, oracle):
    """120 MB of zeros at -9 are three blocks, the first two of 45.9 MB (the bound is 46.6): a staging pass holds one."""
    total = 120_000_000
    z = bz2.compress(bytes(total), 9)
    e, n, info = clean_index(gpu16, z, bytes(total))
    assert n == 3 and e[0].out_len + e[1].out_len > 48 << 20
    crc_bit = e[1].bit + 48 + 13
    entries, nblk, inf, gaps = salvaged(gpu16, flip(z, crc_bit))
    assert [entries[i].key() for i in range(nblk)] == resummed(e, [0, 2])
    assert info_key(inf) == (len(z), total - e[1].out_len, 2, 1)
    assert gaps == [(e[1].bit, e[2].bit, e[0].out_len, 1, GAP_BLOCK_CRC)]
    rc, got, _, _ = gpu16.range_buffer(z, 0, entries, nblk, e[0].out_len - 5, 10)
    assert rc == 0 and got == bytes(10)


@pytest.mark.gpu
def test_gpu_salvage_clean(gpu16, oracle):
    inputs = [(name, z) for name, z, _, _ in index_inputs(oracle)]
    raw = text(oracle, 3 << 20, 304)
    inputs += [("3 MiB of text, level 1", bz2.compress(raw, 1)), ("two streams", bz2.compress(raw[:700_000], 9) + bz2.compress(raw, 2))]
    for name, z in inputs:
        rc, e, info = gpu16.index_build(z)
        assert rc == 0, name
        entries, nblk, inf, gaps = salvaged(gpu16, z, cuts=((7, 16), (1 << 16, 1 << 18)) if len(z) < 4096 else ((1 << 16, 1 << 18),))
        assert bytes(entries)[:40 * nblk] == bytes(e)[:40 * info.nblk] and info_key(inf) == info_key(info), name
        if "stray magic" in name:
            assert len(gaps) == 1 and gaps[0][1] == 8 * len(z) and gaps[0][3] == 1
        else:
            assert gaps == [], (name, gaps)
    for case in reason_cases(oracle) + stream_cases(oracle) + [rounds_case(oracle)]:
        streams = 0 if "truncated" in case[0] else 3 if "three" in case[0] else 1
        entries, n = check_case(gpu16, case, streams, cuts=[(7, 16)])
        check_reading(gpu16, case, entries, n)


@pytest.mark.gpu
def test_gpu_salvage_every_bit_of_one_block(gpu16, oracle):
    """All 363 flips of test_emu_salvage_every_bit_of_one_block."""
    s, bits = every_bit_flips(oracle)
    n = [len(b.raw()) for b in s.blocks]
    keys = s.keys([0, 2, 3])
    for bit in bits:
        rc, entries, info, gaps, ng = gpu16.salvage_build(flip(s.z, bit))
        assert rc == 0
        assert [entries[i].key() for i in range(info.nblk)] == keys, bit
        in_magic = bit < s.magic[1] + 48
        assert ng == 1 and gaps[0][:4] == (s.magic[1], s.magic[2], n[0], 0 if in_magic else 1), (bit, gaps)
        assert info_key(info) == (len(s.z), sum(n) - n[1], 3, 1)
