"""Batched decompression (bzx_decompress_batch_*): many .bz2 inputs decoded in one call.

The rule for every input: given enough room, its output and status are what bzx_decompress_buffer returns for that
input alone -- the same decoder with count = 1, so this is a test of isolation -- and what libbz2 (Python's bz2) says
of it: libbz2 accepts if and only if the status is BZX_OK, with equal bytes.  The documented differences from libbz2
(include/bzx.h) are excepted by name, see documented_difference.
CPU part (-m "not gpu"): the kernels through the fiber emulator (tests/emu), small inputs.
GPU part (-m gpu): the product library on cuda:0."""
import bz2
import ctypes as C
import os
import random
import subprocess

import pytest

import bz2_writer as W
from bzx_ctypes import EMU_PATH, ROOT
from bzx_dbatch_ctypes import DBatchLib

BZX_OK, BZX_E_PARAM, BZX_E_OUTBUF, BZX_E_STATE, BZX_E_DATA = 0, -2, -4, -6, -7


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = DBatchLib(EMU_PATH)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def gpu():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = DBatchLib(max_blocks=16)
    yield lib
    lib.close()


def libbz2(z):
    try:
        return bz2.decompress(z)
    except (OSError, ValueError, EOFError):
        return None


def documented_difference(z, bzh_tail=()):
    """The name of the documented difference from libbz2 that input z falls under, told from its bytes alone (and from
    how the caller built it: bzh_tail), or None.  The library refuses all three kinds."""
    if len(z) < 14:
        return "fewer than 14 bytes"                  # (bz2.decompress(b"") is b""; the other short inputs it refuses too)
    if z[4:10] == W.BLOCK_MAGIC.to_bytes(6, "big") and z[14] & 0x80:
        return "randomised block"                     # the first block's randomised bit (libbz2 decodes short ones)
    if z in bzh_tail:
        return "a BZh<d> after a stream that does not decode"      # (Python's bz2 ignores such a tail)
    return None


def check_equivalent(lib, inputs, rc, got, olen, st, bzh_tail=()):
    """Every input: the batch's verdict and bytes equal bzx_decompress_buffer's on that input alone, and libbz2's
    unless the input is a documented difference; the return value is the lowest failure and the error text names it."""
    err = lib.last_error()
    for k, z in enumerate(inputs):
        rc1, want, n1 = lib.decompress_one(z)
        assert st[k] == rc1, (k, st[k], rc1)
        if rc1 == 0:
            assert got[k] == want and olen[k] == n1, k
        else:
            assert olen[k] == 0 and got[k] is None, k
        if documented_difference(z, bzh_tail):
            assert st[k] == BZX_E_DATA, (k, documented_difference(z, bzh_tail), st[k])
        else:
            py = libbz2(z)
            assert (py is not None) == (st[k] == 0), (k, st[k], None if py is None else len(py))
            assert got[k] == py, k
    bad = [k for k, s in enumerate(st) if s]
    assert rc == (st[bad[0]] if bad else 0)
    if bad:
        assert f"input {bad[0]}:" in err, err


def text(o, n, seed=1):
    return o.synthtext(n, seed=0x9E3779B97F4A7C15 + seed)


def ptext(o, n, period=700, seed=1):
    return (text(o, period, seed) * (n // period + 1))[:n]


# ---- 1. a mixed batch -------------------------------------------------------------------------------------------
def mixed(o):
    t = text(o, 5000, 3)
    multi = W.write_stream(o, [W.Block(ptext(o, 1200, 300, 4)), W.Block(b"Q"), W.Block(ptext(o, 900, 200, 5))], 1)
    three = bz2.compress(t[:700], 2) + bz2.compress(b"", 9) + bz2.compress(t[700:1500], 7)
    return [bz2.compress(t, 1), bz2.compress(t[:3000], 5), bz2.compress(t, 9), bz2.compress(b"", 9), multi, three,
            bz2.compress(t[:400], 9) + b"not a stream, just trailing bytes", bz2.compress(b"x", 3)]


def test_emu_dbatch_mixed(emu, oracle):
    inputs = mixed(oracle)
    assert len(inputs[3]) == 14
    rc, got, olen, st = emu.dbatch_buffer(inputs)
    assert rc == 0 and st == [0] * len(inputs), emu.last_error()
    check_equivalent(emu, inputs, rc, got, olen, st)


# ---- 2. damage and isolation --------------------------------------------------------------------------------------
def refused_shapes(o):
    img = ptext(o, 600, 250, 7)
    L, orig, mtfv, freq, in_use, niu = W.analyse(o, img)
    ng, sel, lens, _ = o.huff(mtfv, freq, niu + 2)
    t21 = [list(x) for x in lens]
    t21[1][2] = 21
    good = W.write_stream(o, [W.Block(img)], 9)
    flip = bytearray(good)
    flip[10] ^= 0x01                                   # inside the stored block CRC
    out = [b"BZh0" + good[4:], b"BZx9" + good[4:], b"", good[:13],
           W.write_stream(o, [W.Block(img, n_groups=7)], 9),
           W.write_stream(o, [W.Block(img, tables=t21)], 9),
           W.write_stream(o, [W.Block(text(o, 300, 9) + b"zzzz")], 9),
           W.write_stream(o, [W.Block(text(o, 150, 31), randomised=1)], 9),
           good[:len(good) // 2], good[:len(good) - 3], bytes(flip),
           good + b"BZh9" + bytes(range(40))]
    return good, out


def test_emu_dbatch_damage_isolated(emu, oracle):
    good, bad = refused_shapes(oracle)
    t = text(oracle, 2000, 11)
    goods = [bz2.compress(t[:200 + 90 * k], 1 + k % 9) for k in range(len(bad) + 1)]
    inputs = []
    for g, b in zip(goods, bad + [None]):
        inputs.append(g)
        if b is not None:
            inputs.append(b)
    rc, got, olen, st = emu.dbatch_buffer(inputs)
    for k, z in enumerate(inputs):
        assert st[k] == (BZX_E_DATA if k % 2 else BZX_OK), (k, st[k])
    assert rc == BZX_E_DATA and "input 1:" in emu.last_error()
    check_equivalent(emu, inputs, rc, got, olen, st, bzh_tail=bad[-1:])
    for k in range(0, len(inputs), 2):
        assert got[k] == bz2.decompress(inputs[k])


# ---- 3. seeded equivalence ---------------------------------------------------------------------------------------
def seeded(o, n, seed, big=False):
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        raw = text(o, rnd.randrange(1, 30000 if big else 1500), seed + k) if k % 3 else rnd.randbytes(rnd.randrange(0, 600))
        z = bz2.compress(raw, rnd.randrange(1, 10))
        kind = rnd.randrange(4)
        if kind == 1:
            zz = bytearray(z)
            bit = rnd.randrange(len(z) * 8)
            zz[bit >> 3] ^= 0x80 >> (bit & 7)
            z = bytes(zz)
        elif kind == 2:
            z = z[:rnd.randrange(len(z))]
        out.append(z)
    return out


def test_emu_dbatch_seeded(emu, oracle):
    inputs = seeded(oracle, 40, 101)
    rc, got, olen, st = emu.dbatch_buffer(inputs)
    check_equivalent(emu, inputs, rc, got, olen, st)


# ---- 4. memory neighbours ------------------------------------------------------------------------------------------
def neighbours(lib, o, device):
    s = bz2.compress(text(o, 3000, 21), 9)
    s2 = bz2.compress(text(o, 2000, 22), 4)
    for parts in ([s[:len(s) // 2], s[len(s) // 2:]], [s[:len(s) - 1], s[len(s) - 1:]], [s, s2], [s2, s]):
        host = C.create_string_buffer(b"".join(parts), sum(map(len, parts)) + 16)
        base = C.addressof(host)
        ptrs = [base, base + len(parts[0])]
        caps = [1 << 16, 1 << 16]
        outs = [C.create_string_buffer(caps[0] + 16) for _ in parts]
        op = [(C.addressof(b) + 15) // 16 * 16 for b in outs]
        call = lib.dbatch_device_raw if device else lib.dbatch_buffer_raw
        rc, olen, st = call(ptrs, [len(p) for p in parts], op, caps)
        for k, z in enumerate(parts):
            rc1, want, n1 = lib.decompress_one(z)
            assert st[k] == rc1, (k, st, rc1)
            if rc1 == 0:
                assert C.string_at(op[k], olen[k]) == want


def test_emu_dbatch_neighbours(emu, oracle):
    neighbours(emu, oracle, False)
    neighbours(emu, oracle, True)            # (the emulator's device memory is host memory)


# ---- 5. output too small -------------------------------------------------------------------------------------------
def outbuf(lib, o):
    t = text(o, 4000, 41)
    inputs = [bz2.compress(t[:1000 + 500 * k], 9) for k in range(5)] + [bz2.compress(b"", 9)]
    sizes = [1000 + 500 * k for k in range(5)] + [0]
    caps = [n - 1 if k in (1, 3) else n for k, n in enumerate(sizes)]
    bufs = [C.create_string_buffer(b"\xa5" * (c + 64), c + 64) for c in caps]
    srcs = [C.create_string_buffer(z, len(z)) for z in inputs]
    outs = [C.addressof(b) if c else None for b, c in zip(bufs, caps)]
    rc, olen, st = lib.dbatch_buffer_raw([C.addressof(s) for s in srcs], [len(z) for z in inputs], outs, caps)
    assert st == [0, BZX_E_OUTBUF, 0, BZX_E_OUTBUF, 0, 0], st
    assert rc == BZX_E_OUTBUF and "input 1:" in lib.last_error()
    assert olen == sizes
    for k in range(5):
        if k in (1, 3):
            assert bufs[k].raw == b"\xa5" * (caps[k] + 64)            # not written
        else:
            assert bufs[k].raw[:sizes[k]] == t[:sizes[k]] and bufs[k].raw[sizes[k]:] == b"\xa5" * 64


def test_emu_dbatch_outbuf(emu, oracle):
    outbuf(emu, oracle)


# ---- 6. arguments -----------------------------------------------------------------------------------------------
def test_emu_dbatch_args(emu, oracle):
    L = emu.lib
    assert L.bzx_decompress_batch_buffer(emu.ctx, 0, None, None, None, None, None, None) == 0
    z = bz2.compress(b"hello", 9)
    rc, olen, st = emu._call(L.bzx_decompress_batch_buffer, [None], [len(z)], [None], [0], arrays=False)
    assert rc == BZX_E_PARAM and st == [BZX_E_PARAM]
    src = C.create_string_buffer(z, len(z))
    out = C.create_string_buffer(64)
    a = (C.addressof(out) + 15) // 16 * 16
    rc, olen, st = emu.dbatch_device_raw([C.addressof(src)] * 2, [len(z)] * 2, [a, a + 1], [16, 16])
    assert rc == BZX_E_PARAM and st == [BZX_E_PARAM] * 2 and "16-byte aligned" in emu.last_error()
    rc, olen, st = emu.dbatch_buffer_raw([C.addressof(src)] * 2, [len(z)] * 2, [a, None], [16, 16])
    assert rc == BZX_E_PARAM and st == [BZX_E_PARAM] * 2
    rc, got, olen, st = emu.dbatch_buffer([z])                  # the context works afterwards
    assert rc == 0 and got == [b"hello"]


# ---- 7. rounds ---------------------------------------------------------------------------------------------------
def rounds_inputs(o):
    five = W.write_stream(o, [W.Block(ptext(o, 300 + 50 * k, 120, 60 + k)) for k in range(5)], 1)
    inputs = [bz2.compress(text(o, 100 + 40 * k, 70 + k), 1 + k % 9) for k in range(9)]
    inputs.insert(4, five)
    inputs.insert(7, bz2.compress(text(o, 300, 90), 3) + bz2.compress(text(o, 200, 91), 8))
    return inputs


def test_emu_dbatch_rounds(oracle):
    inputs = rounds_inputs(oracle)
    small = DBatchLib(EMU_PATH, max_blocks=2)
    wide = DBatchLib(EMU_PATH, max_blocks=16)
    try:
        a = small.dbatch_buffer(inputs)
        b = wide.dbatch_buffer(inputs)
        assert a == b and a[0] == 0, small.last_error()
        assert a[1] == [bz2.decompress(z) for z in inputs]
        st = small.stats()
        assert st.nblk == 9 + 5 + 2
        assert st.raw_bytes == sum(map(len, a[1]))
        assert small.block_info_rc() == BZX_E_STATE
        assert small.decompress_one(inputs[4])[1] == a[1][4]
        assert bz2.decompress(small.compress_buffer(b"after the batch", 9)) == b"after the batch"
    finally:
        small.close()
        wide.close()


# ---- GPU -------------------------------------------------------------------------------------------------------------
def content(o, rnd, k, n):
    kind = k % 4
    return (text(o, n, k) if kind == 0 else rnd.randbytes(n) if kind == 1 else bytes(n) if kind == 2 else
            b"".join(bytes([rnd.randrange(256)]) * rnd.randrange(1, 300) for _ in range(n // 150 + 1))[:n])


@pytest.mark.gpu
def test_gpu_dbatch_2000(gpu, oracle):
    import torch
    rnd = random.Random(5)
    raws = [content(oracle, rnd, k, rnd.randrange(0, 40000)) for k in range(2000)]
    for level in (9, 1):
        streams = gpu.batch_buffer(raws, level)
        rc, got, olen, st = gpu.dbatch_buffer(streams, caps=[len(x) for x in raws])
        assert rc == 0, gpu.last_error()
        assert got == raws
        # the device form: torch views into one allocation (inputs at any byte, outputs on 16-byte boundaries)
        offs, at = [], 0
        for z in streams:
            offs.append(at)
            at += len(z) + 3
        dev_in = torch.zeros(at + 16, dtype=torch.uint8, device="cuda")
        host = bytearray(at + 16)
        for z, o in zip(streams, offs):
            host[o:o + len(z)] = z
        dev_in.copy_(torch.frombuffer(host, dtype=torch.uint8))
        oo, t = [], 0
        for x in raws:
            oo.append(t)
            t += (len(x) + 15) // 16 * 16
        dev_out = torch.zeros(t + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, olen2, st2 = gpu.dbatch_device_raw([dev_in.data_ptr() + o for o in offs], [len(z) for z in streams],
                                               [dev_out.data_ptr() + o if len(x) else None for o, x in zip(oo, raws)],
                                               [len(x) for x in raws])
        assert rc == 0 and st2 == [0] * len(raws), gpu.last_error()
        outb = dev_out.cpu().numpy().tobytes()
        assert [outb[o:o + n] for o, n in zip(oo, olen2)] == raws


@pytest.mark.gpu
def test_gpu_dbatch_full_blocks(gpu, oracle):
    rnd = random.Random(9)
    raws = [text(oracle, 2_500_000, 1), rnd.randbytes(2 << 20), bytes(3 << 20),
            content(oracle, rnd, 3, 2_200_000)]
    inputs = [bz2.compress(x, 9) for x in raws]
    big = text(oracle, 24 * 900_000, 2)
    inputs.append(b"".join(bz2.compress(big[k * 900_000:(k + 1) * 900_000], 9) for k in range(24)))
    raws.append(big)
    rc, got, olen, st = gpu.dbatch_buffer(inputs, caps=[len(x) for x in raws])
    assert rc == 0 and got == raws, gpu.last_error()


@pytest.mark.gpu
def test_gpu_dbatch_damage_and_seeded(gpu, oracle):
    good, bad = refused_shapes(oracle)
    fulls = [W.write_stream(oracle, [W.Block(ptext(oracle, 900_001, 1200, 3))], 9),
             W.write_stream(oracle, [W.Block(ptext(oracle, 100_000, 700, 4) + b"zzzz")], 1)]
    goods = [bz2.compress(text(oracle, 400_000 + k, k), 9) for k in range(len(bad) + len(fulls) + 1)]
    inputs = []
    for g, b in zip(goods, bad + fulls + [None]):
        inputs.append(g)
        if b is not None:
            inputs.append(b)
    rc, got, olen, st = gpu.dbatch_buffer(inputs)
    assert [s != 0 for s in st] == [k % 2 == 1 for k in range(len(inputs))], st
    check_equivalent(gpu, inputs, rc, got, olen, st, bzh_tail=bad[-1:])
    inputs = seeded(oracle, 200, 7, big=True)
    rc, got, olen, st = gpu.dbatch_buffer(inputs)
    check_equivalent(gpu, inputs, rc, got, olen, st)
    outbuf(gpu, oracle)
    neighbours(gpu, oracle, False)


@pytest.mark.gpu
def test_gpu_dbatch_rounds(oracle):
    lib = DBatchLib(max_blocks=4)
    try:
        ten = bz2.compress(text(oracle, 10 * 100_000 - 50_000, 5), 1)
        inputs = [bz2.compress(text(oracle, 50_000 + k, k), 1 + k % 9) for k in range(12)]
        inputs.insert(5, ten)
        rc, got, olen, st = lib.dbatch_buffer(inputs)
        assert rc == 0 and got == [bz2.decompress(z) for z in inputs], lib.last_error()
        s = lib.stats()
        assert s.nblk == 12 + 10 and s.raw_bytes == sum(map(len, got))
        assert lib.block_info_rc() == BZX_E_STATE
    finally:
        lib.close()
