"""Batched compression (bzx_compress_batch_*): many independent inputs, one .bz2 stream each.

CPU part (-m "not gpu"): the kernels through the fiber emulator (tests/emu), as test_emu_kernels.py does.
GPU part (-m gpu): the product library on cuda:0.  Every stream is checked against libbz2 (bz2.compress)."""
import bz2
import ctypes as C
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from bzx_batch_ctypes import BatchLib
from bzx_ctypes import EMU_PATH, ROOT, BzxError

BZX_E_PARAM, BZX_E_OUTBUF, BZX_E_STATE = -2, -4, -6


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = BatchLib(EMU_PATH)
    yield lib
    lib.close()


def want_all(inputs, level):
    with ThreadPoolExecutor(16) as ex:           # bz2 releases the GIL while it compresses
        return list(ex.map(lambda x: bz2.compress(x, level), inputs))


def check_layout(buf, offs, lens):
    """Offsets ascend, start on 4-byte boundaries, streams do not overlap, and the bytes between them are zero."""
    end = 0
    for o, n in zip(offs, lens):
        assert o % 4 == 0 and o >= end, (o, end)
        assert buf[end:o] == bytes(o - end)
        end = o + n


def runs_cases(oracle):
    text = oracle.synthtext(2000)
    out = []
    for n in (3, 4, 5, 255, 256, 1000):
        out += [b"a" * n + text, text + b"z" * n, bytes([n & 255]) * n]
    return out


def mixed_inputs(oracle):
    rnd = random.Random(7)
    return [b"", b"x", b"banana", oracle.synthtext(30000), rnd.randbytes(20000), b"", oracle.synthtext(777)] + runs_cases(oracle)


@pytest.mark.parametrize("level", [1, 9])
def test_emu_batch_mixed(emu, oracle, level):
    inputs = mixed_inputs(oracle)
    streams, buf, offs, lens = emu.batch_buffer(inputs, level, whole=True)
    assert streams == want_all(inputs, level)
    assert streams[0] == bz2.compress(b"", level) and len(streams[0]) == 14
    check_layout(buf, offs, lens)


def test_emu_batch_neighbours(emu, oracle):
    """Input A ends in "aaa", input B starts with "a", back to back in one host buffer (and, A being a multiple of 16
    bytes long, on the device too): a run merged across the two, or a read of the byte before B, changes B's stream."""
    text = oracle.synthtext(4093)
    a = text + b"aaa"                              # 4096 bytes
    for b in (b"a", b"aaaa" + text, b"a" * 300, b"ab" + text):
        host = C.create_string_buffer(a + b, len(a) + len(b))
        base = C.addressof(host)
        out = C.create_string_buffer(emu.batch_bound([len(a), len(b)]))
        rc, offs, lens = emu.batch_buffer_raw([base, base + len(a)], [len(a), len(b)], 9, out, len(out))
        assert rc == 0, emu.last_error()
        raw = out.raw
        assert [raw[o:o + n] for o, n in zip(offs, lens)] == [bz2.compress(a, 9), bz2.compress(b, 9)]


def test_emu_batch_multiblock_and_rounds(oracle):
    """An input a little over two level-1 blocks; a context of 16 slabs with 40 inputs (several device rounds)."""
    lib = BatchLib(EMU_PATH, max_blocks=16)
    try:
        big = oracle.synthtext(2 * 99981 + 500)
        inputs = [oracle.synthtext(1000 + 37 * i, seed=i + 1) for i in range(40)]
        inputs[17] = big
        inputs[30] = b""
        streams, buf, offs, lens = lib.batch_buffer(inputs, 1, whole=True)
        assert streams == want_all(inputs, 1)
        check_layout(buf, offs, lens)
        st = lib.stats()
        assert st.nblk == 39 + 2                   # 38 one-block inputs, one empty, the big one in three blocks
        assert st.raw_bytes == sum(map(len, inputs))
        assert st.out_bits == 8 * sum(lens)
        assert st.rle1_bytes == sum(len(blk) for x in inputs for blk, _ in oracle.split_rle1(x, 1))
    finally:
        lib.close()


def test_emu_batch_device_pointers(emu, oracle):
    """The _device form (the emulator's device memory is host memory): aligned views of one buffer; a misaligned
    pointer is refused and named."""
    inputs = [oracle.synthtext(5000), b"", b"q" * 999, oracle.randbytes(3000)]
    at, n = [], 0
    for x in inputs:
        at.append(n)
        n += (len(x) + 15) // 16 * 16
    raw = C.create_string_buffer(n + 16)
    base = (C.addressof(raw) + 15) // 16 * 16
    for x, o in zip(inputs, at):
        C.memmove(base + o, x, len(x))
    lens = [len(x) for x in inputs]
    cap = emu.batch_bound(lens)
    out = C.create_string_buffer(cap + 16)
    d_out = (C.addressof(out) + 3) // 4 * 4
    ptrs = [base + o if len(x) else None for x, o in zip(inputs, at)]
    offs, olen = emu.batch_device(ptrs, lens, 9, d_out, cap)
    assert [C.string_at(d_out + o, k) for o, k in zip(offs, olen)] == want_all(inputs, 9)
    bad = list(ptrs)
    bad[3] += 1
    rc, _, _ = emu.batch_device_raw(bad, lens, 9, d_out, cap)
    assert rc == BZX_E_PARAM and "input 3" in emu.last_error()
    rc, _, _ = emu.batch_device_raw(ptrs, lens, 9, d_out + 2, cap)
    assert rc == BZX_E_PARAM


def test_emu_batch_errors_and_stats(emu, oracle):
    inputs = [oracle.synthtext(20000), b"hello", oracle.randbytes(7000)]
    lens = [len(x) for x in inputs]
    bufs = [C.create_string_buffer(x, len(x)) for x in inputs]
    ptrs = [C.addressof(b) for b in bufs]
    out = C.create_string_buffer(emu.batch_bound(lens))
    for level in (0, 10):
        assert emu.batch_buffer_raw(ptrs, lens, level, out, len(out))[0] == BZX_E_PARAM
    assert emu.lib.bzx_compress_batch_buffer(emu.ctx, 3, None, None, 9, out, len(out), None, None) == BZX_E_PARAM
    rc, _, _ = emu.batch_buffer_raw([ptrs[0], None, ptrs[2]], lens, 9, out, len(out))
    assert rc == BZX_E_PARAM and "input 1" in emu.last_error()
    assert emu.lib.bzx_compress_batch_buffer(emu.ctx, 0, None, None, 9, None, 0, None, None) == 0
    # too small: BZX_E_OUTBUF, then a correct call on the same context
    rc, _, _ = emu.batch_buffer_raw(ptrs, lens, 9, out, 200)
    assert rc == BZX_E_OUTBUF
    with pytest.raises(BzxError):
        emu.batch_buffer(inputs, 9, cap=sum(len(bz2.compress(x, 9)) for x in inputs) - 8)
    streams = emu.batch_buffer(inputs, 9)
    assert streams == want_all(inputs, 9)
    st = emu.stats()
    assert (st.nblk, st.raw_bytes, st.out_bits) == (3, sum(lens), 8 * sum(map(len, streams)))
    assert st.rle1_bytes == sum(lens) and st.mtf_symbols > 0
    assert emu.block_info_rc(0) == BZX_E_STATE
    # the context still serves the other entry points, and block figures come back after them
    assert emu.compress_buffer(inputs[0], 9) == bz2.compress(inputs[0], 9)
    assert emu.block_info_rc(0) == 0
    assert emu.batch_bound([0, 1, 100]) == 4096 + 4100 + 4200


# ---------------------------------------------------------------------------------------------------- GPU part
@pytest.fixture(scope="module")
def gpu():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = BatchLib()
    yield lib
    lib.close()


def gen_inputs(seed, n, max_len, oracle):
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        k = rnd.randrange(max_len + 1)
        kind = rnd.randrange(4)
        if kind == 0:
            x = oracle.synthtext(k, seed=seed * 100003 + i + 1)
        elif kind == 1:
            x = rnd.randbytes(k)
        elif kind == 2:
            x = bytes(k)
        else:
            x = b"".join(bytes([rnd.randrange(256)]) * rnd.choice((1, 3, 4, 5, 200, 255, 256, 600)) for _ in range(k // 50 + 1))[:k]
        out.append(x)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("level", [1, 5, 9])
def test_gpu_batch_2000_inputs(gpu, oracle, level):
    inputs = gen_inputs(level, 2000, 300_000, oracle)
    streams, buf, offs, lens = gpu.batch_buffer(inputs, level, whole=True)
    assert streams == want_all(inputs, level)
    check_layout(buf, offs, lens)
    st = gpu.stats()
    assert st.raw_bytes == sum(map(len, inputs)) and st.out_bits == 8 * sum(lens) and st.ms_total > 0


@pytest.mark.gpu
def test_gpu_batch_large_and_periodic(gpu, oracle):
    rnd = random.Random(11)
    inputs = []
    for i in range(60):
        inputs.append(oracle.synthtext(rnd.randrange(1, 3000), seed=i + 5))
        if i % 20 == 0:
            inputs.append(oracle.synthtext(3_000_000, seed=i + 99))
    inputs.insert(31, bytes(255 * 3530))           # 900 KB of zeros: RLE1 makes 3530 equal pieces, a periodic block
    for level in (9, 2):
        assert gpu.batch_buffer(inputs, level) == want_all(inputs, level)
        assert gpu.stats().n_periodic == 1


@pytest.mark.gpu
def test_gpu_batch_device_views(gpu, oracle):
    """bzx_compress_batch_device on views of one torch uint8 tensor at 16-byte aligned offsets; every stream equals
    bzx_compress_device of the same input on the same context; a misaligned view is refused."""
    import torch
    inputs = gen_inputs(42, 300, 200_000, oracle) + [oracle.synthtext(2_500_000)]
    at, n = [], 0
    for x in inputs:
        at.append(n)
        n += (len(x) + 15) // 16 * 16 + 16 * random.Random(len(x)).randrange(3)
    host = bytearray(n)
    for x, o in zip(inputs, at):
        host[o:o + len(x)] = x
    d_in = torch.frombuffer(host, dtype=torch.uint8).to("cuda")
    lens = [len(x) for x in inputs]
    cap = gpu.batch_bound(lens)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ptrs = [d_in.data_ptr() + o if len(x) else None for x, o in zip(inputs, at)]
    torch.cuda.synchronize()
    offs, olen = gpu.batch_device(ptrs, lens, 9, d_out.data_ptr(), cap)
    outb = d_out.cpu().numpy().tobytes()
    streams = [outb[o:o + k] for o, k in zip(offs, olen)]
    assert streams == want_all(inputs, 9)
    check_layout(outb, offs, olen)
    one = torch.zeros(max(lens) + max(lens) // 50 + 4096, dtype=torch.uint8, device="cuda")
    for i in range(0, len(inputs), 25):
        k = gpu.compress_device(ptrs[i] or d_in.data_ptr(), lens[i], 9, one.data_ptr(), one.numel())
        assert one[:k].cpu().numpy().tobytes() == streams[i], i
    bad = list(ptrs)
    j = next(i for i, x in enumerate(inputs) if len(x))
    bad[j] += 4
    rc, _, _ = gpu.batch_device_raw(bad, lens, 9, d_out.data_ptr(), cap)
    assert rc == BZX_E_PARAM and f"input {j}" in gpu.last_error()


@pytest.mark.gpu
def test_gpu_batch_rounds_then_other_entry_points(oracle):
    """Several device rounds on a context of 16 slabs; then bzx_compress_device and the chunked stream on it."""
    import torch
    torch.cuda.init()
    lib = BatchLib(max_blocks=16)
    try:
        inputs = gen_inputs(5, 100, 120_000, oracle) + [oracle.synthtext(20 * 900_000 + 5)]   # one input of 21 blocks
        assert lib.batch_buffer(inputs, 9) == want_all(inputs, 9)
        with pytest.raises(BzxError):
            lib.batch_buffer(inputs, 9, cap=1000)
        assert lib.batch_buffer(inputs[:50], 3) == want_all(inputs[:50], 3)
        data = oracle.synthtext(3_000_000) + bytes(10_000)
        d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
        d_out = torch.zeros(len(data) + len(data) // 50 + 4096, dtype=torch.uint8, device="cuda")
        k = lib.compress_device(d_in.data_ptr(), len(data), 9, d_out.data_ptr(), d_out.numel())
        assert d_out[:k].cpu().numpy().tobytes() == bz2.compress(data, 9)
        assert lib.cstream_compress(data, 9, chunk=1 << 20) == bz2.compress(data, 9)
        assert lib.batch_buffer(inputs[50:], 9) == want_all(inputs[50:], 9)
    finally:
        lib.close()
