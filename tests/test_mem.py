"""GPU part (-m gpu) of the memory owners (csrc/bzx_mem.h): the buffers a context grows on demand, each used below its
floor, then forced to grow, then used small again -- on ONE context, every step checked against libbz2.  The
allocation-failure paths and the balance of allocations and frees are the emulator's part (tests/test_emu_mem.py)."""
import bz2
import random

import pytest

from bzx_dstream_ctypes import dstream_decode
from bzx_ranges_ctypes import RangesLib


def read(lib, z, entries, n, ranges, want):
    r = lib.ranges_buffer(z, None, entries, n, ranges)
    assert r.rc == 0 and r.status == [0] * len(ranges), lib.last_error()
    assert [r.data(i) for i in range(len(ranges))] == [want[o:o + w] for o, w in ranges]


@pytest.mark.gpu
def test_gpu_mem_grow_and_reuse(oracle):
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = RangesLib(max_blocks=16)
    try:
        texts = [oracle.synthtext(900 + 7 * i, seed=100 + i) for i in range(40)]
        zs = [bz2.compress(t, 9) for t in texts]
        # batched decompression: dbatch_pin[0], dbatch_pin[1] and dbatch_ws grow with count
        for k in (2, 40, 2):
            rc, got, olen, st = lib.dbatch_buffer(zs[:k], caps=[2048] * k)
            assert rc == 0 and st == [0] * k and got == texts[:k], (k, lib.last_error())
        # batched compression: batch_ws grows with count
        for k in (2, 40, 2):
            assert lib.batch_buffer(texts[:k], 9) == zs[:k], k
        # range reads, 5 MiB of zeros (one block, under 100 compressed bytes): the whole output is over rg_io's 4 MiB floor
        zeros = bytes(5 << 20)
        z = bz2.compress(zeros, 9)
        assert len(z) < 100
        rc, entries, info = lib.index_build(z)
        assert rc == 0 and info.nblk == 1, lib.last_error()
        for ranges in ([(1000, 64)], [(0, len(zeros))], [(1000, 64)]):
            read(lib, z, entries, 1, ranges, zeros)
        # range reads, three blocks of text: 5000 ranges of 1 to 3 bytes are over the slice table's 4096-entry floor
        text = oracle.synthtext(250_000, seed=7)
        z = bz2.compress(text, 1)
        rc, entries, info = lib.index_build(z)
        assert rc == 0 and info.nblk == 3, lib.last_error()
        rnd = random.Random(5)
        many = [(rnd.randrange(len(text) - 3), rnd.randrange(1, 4)) for _ in range(5000)]
        for ranges in ([(12345, 10)], many, [(12345, 10)]):
            read(lib, z, entries, 3, ranges, text)
        # the streaming decompressor twice, a one-shot call between: the second stream holds what the first held
        figures = []
        for k in range(2):
            rc, got, info = dstream_decode(lib, zs[0] + zs[1], 700, 4096, max_chunk=65536)
            assert rc == 0 and got == texts[0] + texts[1]
            figures.append((info.device_bytes, info.pinned_bytes))
            if k == 0:
                rc, got, _ = lib.decompress_one(zs[2], cap=4096)
                assert rc == 0 and got == texts[2]
        assert figures[0] == figures[1] and figures[0][0] > 0 and figures[0][1] > 0
    finally:
        lib.close()
