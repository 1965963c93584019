"""Streaming decompression (bzx_dstream_*): the .bz2 fed in pieces, the output taken in pieces, bounded device memory.

The rule: for any way of cutting the input into feed calls and any sequence of cap values, the concatenated output and
the final status are what bzx_decompress_buffer returns for the whole input (and libbz2's bytes where it accepts it).
CPU part (-m "not gpu"): the whole state machine and its kernels through the fiber emulator (tests/emu), small inputs.
GPU part (-m gpu): the product library on cuda:0, real sizes."""
import bz2
import ctypes as C
import hashlib
import os
import random
import subprocess

import pytest

import bz2_writer as W
from bzx_ctypes import EMU_PATH, ROOT
from bzx_dstream_ctypes import DStreamLib, dstream_decode

BZX_OK, BZX_E_PARAM, BZX_E_STATE, BZX_E_DATA = 0, -2, -6, -7
BLOCK_MAGIC = bytes.fromhex("314159265359")
BIG = 1 << 20


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = DStreamLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


def text(o, n, seed=1):
    return o.synthtext(n, seed=0x9E3779B97F4A7C15 + seed)


def ptext(o, n, period=700, seed=1):
    return (text(o, period, seed) * (n // period + 1))[:n]


def text_class(msg):
    """What kind of refusal an error text names."""
    if "randomised" in msg:
        return "randomised"
    if "CRC" in msg:
        return "crc"
    return "structure"                   # header, truncation, damaged block, blocks that do not end at a marker


_one_shot = {}


def one_shot(lib, z):
    """bzx_decompress_buffer on the whole input: (rc, bytes or None, class of the error text)."""
    key = (id(lib), bytes(z))
    if key not in _one_shot:
        rc, want, _ = lib.decompress_one(z, cap=max(60 * len(z), BIG))
        _one_shot[key] = (rc, want, text_class(lib.last_error()) if rc else None)
    return _one_shot[key]


def check_same(lib, z, feeds, caps, max_chunk, bounds=None, truth=None):
    """The stream's verdict and bytes against bzx_decompress_buffer's; after an error the delivered bytes are a
    prefix of `truth` that ends on one of `bounds`.  Returns (rc, bytes, info)."""
    rc, got, info = dstream_decode(lib, z, feeds, caps, max_chunk)
    cls = text_class(lib.last_error()) if rc else None
    rc1, want, cls1 = one_shot(lib, z)
    assert rc == rc1, (rc, rc1, lib.last_error())
    if rc == 0:
        assert got == want
        assert info.out_bytes == len(want) and info.in_bytes <= len(z)
    else:
        assert rc == BZX_E_DATA and cls == cls1, (cls, cls1)
        if truth is not None:
            assert truth.startswith(got) and len(got) in bounds, (len(got), bounds)
    return rc, got, info


# ---- 1. any cutting, same bytes -----------------------------------------------------------------------------------
def cutting_inputs(o):
    """(name, .bz2, blocks, streams)"""
    t = text(o, 1500, 3)
    multi = W.write_stream(o, [W.Block(ptext(o, 500, 170, 4)), W.Block(ptext(o, 400, 130, 5)), W.Block(text(o, 250, 6))], 1)
    three = bz2.compress(t[:500], 2) + bz2.compress(b"", 9) + bz2.compress(t[500:900], 7)
    trailing = bz2.compress(t[:400], 9) + b"xy" + BLOCK_MAGIC + b"..BZh" + b"trailing bytes, no stream"
    one_byte = W.write_stream(o, [W.Block(ptext(o, 300, 110, 7)), W.Block(b"Q"), W.Block(ptext(o, 200, 90, 8))], 9)
    return [("multi-block BZh1", multi, 3, 1), ("level 5", bz2.compress(t[:1200], 5), 1, 1),
            ("level 9", bz2.compress(t[:900], 9), 1, 1), ("empty", bz2.compress(b"", 9), 0, 1),
            ("three streams, the middle one empty", three, 2, 3), ("trailing magic and BZh", trailing, 1, 1),
            ("a one-byte block", one_byte, 3, 1)]


def test_emu_dstream_any_cutting(emu, oracle):
    rnd = random.Random(5)
    combo = 0
    for name, z, nblk, nstreams in cutting_inputs(oracle):
        want = bz2.decompress(z)
        plans = [(f, c) for f in (1, 7, 4096, 0) for c in (1, 100, BIG)]
        plans.append((lambda: rnd.choice((1, 2, 7, 64, 300, 4096)), lambda: rnd.choice((1, 3, 100, 777, BIG))))
        for feeds, caps in plans:
            max_chunk = (64, 256, 1 << 16)[combo % 3]
            combo += 1
            rc, got, info = check_same(emu, z, feeds, caps, max_chunk)
            assert rc == 0 and got == want, (name, feeds, caps, max_chunk, emu.last_error())
            assert (info.nblk, info.nstreams) == (nblk, nstreams), (name, info.nblk, info.nstreams)
            st = emu.stats()
            assert st.nblk == nblk and st.raw_bytes == len(want)


# ---- 2. borders ---------------------------------------------------------------------------------------------------
def two_streams(o, sizes=(150, 100, 80)):
    """A two-block BZh1 stream and a one-block BZh9 stream: (.bz2, raw bytes, block boundaries of the output,
    byte positions of the block starts, the end-of-stream markers, the footers and the second header)."""
    b = [W.Block(ptext(o, sizes[0], 60, 21)), W.Block(ptext(o, sizes[1], 45, 22)), W.Block(text(o, sizes[2], 23))]
    f1, f2 = {}, {}
    z1 = W.write_stream(o, b[:2], 1, fields=f1)
    z2 = W.write_stream(o, b[2:], 9, fields=f2)
    raw = b"".join(x.raw() for x in b)
    bounds, n = [0], 0
    for x in b:
        n += len(x.raw())
        bounds.append(n)
    marks = [s // 8 for s, _ in f1["magic"]] + [f1["eos"][0][0] // 8, f1["stream_crc"][0][0] // 8, len(z1)]
    marks += [len(z1) + f2["magic"][0][0] // 8, len(z1) + f2["eos"][0][0] // 8, len(z1) + f2["stream_crc"][0][0] // 8]
    return z1 + z2, raw, bounds, marks, f1


def test_emu_dstream_borders(emu, oracle):
    z, raw, _, marks, _ = two_streams(oracle)
    assert bz2.decompress(z) == raw
    cuts = sorted({m + d for m in marks for d in range(-8, 9) if 1 <= m + d < len(z)})
    assert len(cuts) > 60
    for cut in cuts:
        # the accepted bytes become a window when max_chunk of them are there: the cut is a window border
        rc, got, info = dstream_decode(emu, z, [cut, 0], BIG, max(cut, 16))
        assert rc == 0 and got == raw, (cut, rc, emu.last_error())
        assert (info.nblk, info.nstreams) == (3, 2) and info.windows >= 2, (cut, info.windows)


# ---- 3. damage, same verdict --------------------------------------------------------------------------------------
def damaged_inputs(o):
    z, raw, bounds, marks, f1 = two_streams(o)
    rnd = random.Random(17)
    out = []
    cuts = {2, 3, 9, 13, marks[0] + 30, marks[1] + 25, marks[2] + 2, marks[3] + 1, marks[3] + 3, marks[4] + 2, len(z) - 1,
            len(z) - 5, len(z) - 9}
    cuts |= {rnd.randrange(1, len(z)) for _ in range(6)}
    for c in sorted(cuts):
        out.append((f"truncated at {c}", z[:c]))
    flip = bytearray(z)
    bit = f1["magic"][1][0] + (f1["eos"][0][0] - f1["magic"][1][0]) * 3 // 4         # payload of the second block
    flip[bit >> 3] ^= 0x80 >> (bit & 7)
    out.append(("a payload bit of block 2 flipped", bytes(flip)))
    flip = bytearray(z)
    flip[f1["crc"][1][0] // 8 + 1] ^= 0x10
    out.append(("stored CRC of block 2 damaged", bytes(flip)))
    b = [W.Block(ptext(o, 150, 60, 21)), W.Block(ptext(o, 100, 45, 22))]
    out.append(("combined CRC wrong", W.write_stream(o, b, 1, combined_crc=0x12345678)))
    out.append(("a randomised block", W.write_stream(o, [b[0], W.Block(text(o, 90, 31), randomised=1)], 9)))
    out.append(("a block longer than its level allows", W.write_stream(o, [b[0], W.Block(b"a" * 100001)], 1)))
    out.append(("BZh5 and noise after a good stream", z + b"BZh5" + bytes(range(40))))
    return out, raw, set(bounds)


def test_emu_dstream_damage_same_verdict(emu, oracle):
    cases, raw, bounds = damaged_inputs(oracle)
    seen = set()
    for k, (name, z) in enumerate(cases):
        for feeds, caps, max_chunk in ((0, BIG, 1 << 16), (7, 50, 128)):
            rc, got, _ = check_same(emu, z, feeds, caps, max_chunk, bounds, raw)
            if rc:
                seen.add(text_class(emu.last_error()))
            if "truncated" not in name or len(z) < 14:
                assert rc == BZX_E_DATA, (name, rc)
    assert seen == {"randomised", "crc", "structure"}
    # block 1 had been verified when block 2 failed: it was delivered
    rc, got, _ = dstream_decode(emu, cases[-5][1], 7, 50, 128)
    assert "stored CRC" in cases[-5][0] and rc == BZX_E_DATA and got == raw[:150] and "block 1" in emu.last_error()
    # the context is as good as new
    z = bz2.compress(raw, 3)
    assert dstream_decode(emu, z, 5, 33, 64)[:2] == (0, raw)


# ---- 4. calling rules -----------------------------------------------------------------------------------------------
def test_emu_dstream_calling_rules(emu, oracle):
    raw = text(oracle, 600, 41)
    z = bz2.compress(raw, 9)
    L = emu.lib
    s = emu.dstream(64)
    try:
        assert s.feed(b"", False, 100) == (BZX_OK, 0, b"", 0)                   # nothing happens
        # NULL arguments
        used, made, done = C.c_size_t(), C.c_size_t(), C.c_int()
        buf, out = C.create_string_buffer(z, len(z)), C.create_string_buffer(4096)
        args = [s.h, C.addressof(buf), len(z), 1, C.byref(used), C.addressof(out), 4096, C.byref(made), C.byref(done)]
        for k, v in ((0, None), (1, None), (4, None), (5, None), (7, None), (8, None)):
            a = list(args)
            a[k] = v
            assert L.bzx_dstream_feed(*a) == BZX_E_PARAM, k
        assert L.bzx_dstream_begin(None, 0, C.byref(C.c_void_p())) == BZX_E_PARAM
        assert L.bzx_dstream_begin(emu.ctx, 0, None) == BZX_E_PARAM
        assert L.bzx_dstream_get_info(s.h, None) == BZX_E_PARAM and L.bzx_dstream_get_info(None, None) == BZX_E_PARAM
        L.bzx_dstream_end(None)
        # half of the input, then the context is asked for other work: refused, and the stream goes on
        rc, used1, got1, done1 = s.feed(z[:200], False, 4096)
        assert (rc, used1, done1) == (0, 200, 0)
        other = C.c_void_p()
        assert L.bzx_dstream_begin(emu.ctx, 0, C.byref(other)) == BZX_E_STATE and not other.value
        assert "bzx_dstream" in emu.last_error()
        rc1, _, _ = emu.decompress_one(z)
        assert rc1 == BZX_E_STATE and "bzx_dstream" in emu.last_error()
        with pytest.raises(Exception):
            emu.compress_buffer(raw, 9)
        rc, used2, got2, done2 = s.feed(z[200:], False, 4096)                  # everything fed, final not said yet
        assert (rc, used2) == (0, len(z) - 200)
        got3 = b""
        while not done2:
            rc, used3, more, done2 = s.feed(b"", True, 100)                    # final with len == 0
            assert rc == 0 and used3 == 0 and (more or done2)
            got3 += more
        assert got1 + got2 + got3 == raw
        rc, used4, got4, done4 = s.feed(b"", True, 100)                        # after done
        assert rc == BZX_E_STATE and not used4 and not got4 and not done4
        rc, used4, got4, done4 = s.feed(z, True, 100)
        assert rc == BZX_E_STATE
    finally:
        s.end()
    # after end the context works as before
    assert emu.decompress_one(z)[:2] == (0, raw)
    assert bz2.decompress(emu.compress_buffer(raw, 9)) == raw
    assert dstream_decode(emu, z, 0, BIG)[:2] == (0, raw)
    # more magics in a window than its candidate table holds (here in trailing bytes): the scan halves its range
    rc, got, info = dstream_decode(emu, z + BLOCK_MAGIC * 11000, 0, BIG, 1 << 17)
    assert (rc, got) == (0, raw) and info.windows == 1 and info.scans > 1


# ---- 5. bounded -----------------------------------------------------------------------------------------------------
def many_blocks(o, n, size=200):
    blocks = [W.Block(ptext(o, size + k % 7, 50 + k % 11, 100 + k % 5)) for k in range(n)]
    return W.write_stream(o, blocks, 9), b"".join(b.raw() for b in blocks)


def test_emu_dstream_bounded(emu, oracle):
    figures = []
    for n in (80, 160):
        z, raw = many_blocks(oracle, n)
        rc, got, info = dstream_decode(emu, z, 1000, 3000, 2048)           # (checks the figures before and after)
        assert rc == 0 and got == raw, emu.last_error()
        assert info.slabs == 16 and info.nblk == n and info.nstreams == 1
        assert info.rounds >= n // 16 and info.windows >= len(z) // 2048
        figures.append((info.slabs, info.device_bytes, info.pinned_bytes))
    assert figures[0] == figures[1]                                        # they do not depend on the input


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu16():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = DStreamLib(max_blocks=16)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def maker():
    """A context of its own for making the inputs: compression grows a context's slabs, and the decoding contexts
    are to keep the number they were created with."""
    lib = DStreamLib(max_blocks=16)
    yield lib
    lib.close()


def block_ends(lib):
    """Output offsets at which the blocks of the stream `lib` compressed last end (text without runs of four equal
    bytes: RLE1 is the identity, a block's n is its raw length; libbz2 ends a block at 100000 x level - 19 bytes or up
    to three more)."""
    ends, n = {0}, 0
    for i in range(lib.stats().nblk):
        n += lib.block_info(i).n
        ends.add(n)
    return ends


def decode_hashed(lib, z, feeds, caps, max_chunk):
    h = hashlib.sha256()
    n = [0]

    def sink(piece):
        h.update(piece)
        n[0] += len(piece)
    rc, _, info = dstream_decode(lib, z, feeds, caps, max_chunk, sink=sink)
    return rc, h.hexdigest(), n[0], info


@pytest.mark.gpu
def test_gpu_dstream_any_cutting_real_sizes(gpu16, maker, oracle):
    raw = text(oracle, 16 << 20, 51)
    rnd = random.Random(7)
    for level in (1, 9):
        z = maker.compress_buffer(raw, level)
        nblk = maker.stats().nblk
        assert bz2.decompress(z) == raw and nblk >= len(raw) // (100000 * level)
        for feeds, caps in ((0, 64 << 20), (1 << 20, 1 << 20), (lambda: rnd.randrange(1, 3 << 20), lambda: rnd.randrange(1, 8 << 20)),
                            (65537, 4099)):
            rc, got, info = dstream_decode(gpu16, z, feeds, caps, 4 << 20)
            assert rc == 0 and got == raw, (level, gpu16.last_error())
            assert info.slabs == 16 and info.nstreams == 1 and info.windows >= len(z) // (4 << 20)
            assert info.nblk == nblk
            assert info.rounds >= info.nblk // 16
        rc1, want, _ = maker.decompress_one(z, cap=len(raw) + 64)        # (the one-shot call grows its context)
        assert rc1 == 0 and want == raw
    # the small shapes of the CPU part, on the device
    for name, z, nblk, nstreams in cutting_inputs(oracle):
        for feeds, caps, max_chunk in ((1, 1, 64), (7, 100, 256), (0, BIG, 0)):
            rc, got, info = check_same(gpu16, z, feeds, caps, max_chunk)
            assert rc == 0 and got == bz2.decompress(z) and (info.nblk, info.nstreams) == (nblk, nstreams), name


@pytest.mark.gpu
def test_gpu_dstream_damage_real_sizes(gpu16, maker, oracle):
    cases, raw, bounds = damaged_inputs(oracle)
    for name, z in cases:
        for feeds, caps, max_chunk in ((0, BIG, 0), (7, 50, 128)):
            check_same(gpu16, z, feeds, caps, max_chunk, bounds, raw)
    big = text(oracle, 16 << 20, 52)
    z = maker.compress_buffer(big, 9)
    ends = block_ends(maker)
    assert max(ends) == len(big)
    # truncated inside a block, a flipped bit in the middle of the stream, a wrong combined CRC
    for name, bad in (("cut", z[:len(z) * 2 // 3]), ("cut in the footer", z[:-3]),
                      ("flip", z[:len(z) // 2] + bytes([z[len(z) // 2] ^ 0x04]) + z[len(z) // 2 + 1:]),
                      ("combined", z[:-1] + bytes([z[-1] ^ 0xFF]))):
        rc, got, _ = dstream_decode(gpu16, bad, 1 << 20, 3 << 20, 4 << 20)
        cls = text_class(gpu16.last_error())
        rc1, _, cls1 = one_shot(maker, bad)
        assert rc == rc1 == BZX_E_DATA and cls == cls1, (name, rc, rc1, cls, cls1)
        assert big.startswith(got) and len(got) in ends, (name, len(got))
        if name in ("cut", "flip"):
            assert len(got) >= 5 * 899981
    assert dstream_decode(gpu16, z, 0, 64 << 20, 4 << 20)[:2] == (0, big)


@pytest.mark.gpu
def test_gpu_dstream_expansion(gpu16, maker):
    """256 MiB of zeros: a few hundred bytes of .bz2, where the output and not the blocks cuts the rounds."""
    n = 256 << 20
    z = maker.compress_buffer(bytes(n), 9)
    assert len(z) < 1000
    rc, digest, total, info = decode_hashed(gpu16, z, 0, 1 << 20, 0)
    assert rc == 0 and total == n, gpu16.last_error()
    assert digest == hashlib.sha256(bytes(n)).hexdigest()
    assert info.slabs == 16 and info.windows == 1 and info.rounds >= n // (48 << 20)


@pytest.mark.gpu
def test_gpu_dstream_256mib_text_and_damage(maker, oracle):
    lib = DStreamLib(max_blocks=64)
    try:
        raw = text(oracle, 256 << 20, 53)
        z = maker.compress_buffer(raw, 9)
        ends = sorted(block_ends(maker))
        rnd = random.Random(9)
        want = hashlib.sha256(raw).hexdigest()
        rc, digest, total, info = decode_hashed(lib, z, lambda: rnd.randrange(1, 12 << 20), 16 << 20, 8 << 20)
        assert rc == 0 and total == len(raw) and digest == want, lib.last_error()
        assert info.slabs == 64 and info.nblk == len(ends) - 1 >= 298
        # block 100's payload damaged: the blocks before it are delivered, nothing of it or behind it
        at = len(z) * 100 // info.nblk + len(z) // info.nblk // 2
        bad = z[:at] + bytes([z[at] ^ 0x20]) + z[at + 1:]
        out = []
        rc, _, info = dstream_decode(lib, bad, lambda: rnd.randrange(1, 12 << 20), 16 << 20, 8 << 20, sink=out.append)
        got = b"".join(out)
        assert rc == BZX_E_DATA
        assert len(got) in ends[90:101], len(got)                            # whole blocks, at most 100 of them
        assert raw.startswith(got)
    finally:
        lib.close()


@pytest.mark.gpu
def test_gpu_dstream_2000_blocks_on_16_slabs(gpu16, maker, oracle):
    raw = ptext(oracle, 2000 * 99981 - 5000, 1 << 20, 54)
    z = maker.compress_buffer(raw, 1)
    assert maker.stats().nblk == 2000
    rc, digest, total, info = decode_hashed(gpu16, z, 0, 32 << 20, 16 << 20)
    assert rc == 0 and total == len(raw) and digest == hashlib.sha256(raw).hexdigest(), gpu16.last_error()
    assert info.nblk == 2000 and info.slabs == 16 and info.rounds >= 125
