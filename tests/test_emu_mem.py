"""CPU tests (-m "not gpu"): who frees what, through the fiber emulator (tests/emu).

The emulator's hipMalloc / hipHostMalloc count the live device and pinned allocations and can fail the k-th allocation
from now once (tests/emu/hip_emu.cpp).  Per call family, on a context created inside the test:
  balance  the call gives the right bytes, and after bzx_ctx_destroy both live counts are what they were before;
  sweep    for EVERY k below the allocations a clean run makes (context creation included), the k-th allocation fails:
           the step that met it returns BZX_E_NOMEM with a text, the same call then succeeds on the same context (on a
           new one if it was the creation that failed), and after the destroy the live counts are back.
Inputs are a few hundred bytes: the host paths do not depend on the size.  What the file costs is the emulator's fixed
time per call (0.2 s to decompress, 0.65 s to compress, 1.2 s for a batch, whatever the size) times the one good call
every k of a sweep needs."""
import bz2
import ctypes as C
import os
import random
import subprocess

import pytest

from bzx_ctypes import EMU_PATH, ROOT, BzxError
from bzx_dstream_ctypes import dstream_decode
from bzx_mdev_ctypes import MDev
from bzx_ranges_ctypes import RangesLib
from bzx_salvage_ctypes import SalvageLib
from test_range import py_walk

E_NOMEM = -3
RND = random.Random(11)
TEXT = bytes(RND.choice(b"abcdefgh \n") for _ in range(700)) + b"\0" * 40 + b"tail"
Z = bz2.compress(TEXT, 1)
Z2 = bz2.compress(TEXT[:300], 9)


class Mem:
    """The emulator's allocation counters."""

    def __init__(self):
        self.L = L = C.CDLL(EMU_PATH)
        L.hipemu_mem_live.restype = L.hipemu_mem_total.restype = C.c_long
        L.hipemu_mem_live.argtypes = [C.c_int]
        L.hipemu_mem_fail_after.argtypes = [C.c_long]

    def live(self):
        return self.L.hipemu_mem_live(0), self.L.hipemu_mem_live(1)

    def total(self):
        return self.L.hipemu_mem_total()

    def fail_after(self, k):
        self.L.hipemu_mem_fail_after(k)


@pytest.fixture(scope="module")
def mem():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", f) for f in ("hip/hip_runtime.h", "hip_emu.cpp")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    return Mem()


class Lib(RangesLib, SalvageLib):
    """Every call family of this file on one context."""


@pytest.fixture(scope="module")
def index(mem):
    """The index entries of Z, from a context of their own."""
    lib = Lib(EMU_PATH)
    try:
        rc, entries, info = lib.index_build(Z)
        assert rc == 0 and info.nblk >= 1
        return entries, info.nblk
    finally:
        lib.close()


# ---- the families: f(lib, aux) -> the first failing return code, or 0 after checking what the call delivered ----------
def rc_of(call):
    try:
        return call() or 0
    except BzxError as e:
        return e.code


def f_compress_buffer(lib, aux):
    def go():
        assert lib.compress_buffer(TEXT, 1) == bz2.compress(TEXT, 1)
    return rc_of(go)


def f_compress_batch_buffer(lib, aux):
    inputs = [TEXT, TEXT[:123]]

    def go():
        assert lib.batch_buffer(inputs, 1) == [bz2.compress(x, 1) for x in inputs]
    return rc_of(go)


def f_decompress_buffer(lib, aux):
    rc, got, _ = lib.decompress_one(Z, cap=4096)
    assert rc or got == TEXT
    return rc


def f_decompress_batch_buffer(lib, aux):
    rc, got, olen, st = lib.dbatch_buffer([Z, Z2], caps=[4096, 4096])
    assert rc or (got == [TEXT, TEXT[:300]] and st == [0, 0])
    assert rc == 0 or st == [rc, rc]
    return rc


def f_dstream(lib, aux):
    def go():
        rc, got, info = dstream_decode(lib, Z + Z2, 0, 4096, max_chunk=64)
        assert rc or got == TEXT + TEXT[:300]
        return rc
    return rc_of(go)


def f_index_build(lib, aux):
    rc, entries, info = lib.index_build(Z)
    assert rc or [entries[i].key() for i in range(info.nblk)] == [aux[0][i].key() for i in range(aux[1])]
    return rc


def f_salvage_build(lib, aux):
    """Z is intact: the entries are the index's, and there is no gap."""
    rc, entries, info, gaps, ngaps = lib.salvage_build(Z)
    assert rc or [entries[i].key() for i in range(info.nblk)] == [aux[0][i].key() for i in range(aux[1])]
    assert rc or (gaps == [] and ngaps == 0)
    assert rc == 0 or (info.nblk == 0 and ngaps == 0)        # a failed run hands nothing out
    return rc


def f_salvage_buffer(lib, aux):
    rc, got, out_len, gaps, ngaps = lib.salvage_buffer(Z, 4096)
    assert rc or (got == TEXT and out_len == len(TEXT) and gaps == [] and ngaps == 0)
    return rc


def f_range_buffer(lib, aux):
    rc, got, room, g = lib.range_buffer(Z, 0, aux[0], aux[1], 100, 333)
    assert rc or got == TEXT[100:433]
    return rc


def f_ranges_buffer(lib, aux):
    ranges = [(5, 10), (600, 1000), (0, 0), (300, 77)]
    r = lib.ranges_buffer(Z, None, aux[0], aux[1], ranges)
    assert r.rc or [r.data(i) for i in range(len(ranges))] == [TEXT[o:o + w] for o, w in ranges]
    assert r.rc == 0 or r.status == [r.rc] * len(ranges)
    return r.rc


def f_stage_gather(lib, aux):
    slices = [(3, 1, 200), (0, 300, 45)]
    rc, got = lib.stage_gather(TEXT, slices, b"\xa5" * 400)
    exp = bytearray(b"\xa5" * 400)
    for so, do, ln in slices:
        exp[do:do + ln] = TEXT[so:so + ln]
    assert rc or got == bytes(exp)
    return rc


def f_stage_ibwt(lib, aux):
    oracle = aux[2]
    blk = TEXT[:500]
    L, orig = oracle.bwt(blk)
    img, raw, four = py_walk(L, orig)
    assert img == blk and not four

    def go():
        for wide in (0, 1):
            assert lib.stage_ibwt(L, orig, wide) == (img, raw, len(raw), 0)
    return rc_of(go)


def f_split_rle1(lib, aux):
    def go():
        assert lib.split_rle1(TEXT, 1) == aux[2].split_rle1(TEXT, 1)
    return rc_of(go)


FAMILIES = [f_compress_buffer, f_compress_batch_buffer, f_decompress_buffer, f_decompress_batch_buffer, f_dstream,
            f_index_build, f_salvage_build, f_salvage_buffer, f_range_buffer, f_ranges_buffer, f_stage_gather, f_stage_ibwt, f_split_rle1]


def create():
    """-> (lib, 0), or (None, the code bzx_ctx_create returned)"""
    try:
        return Lib(EMU_PATH), 0
    except BzxError as e:
        return None, e.code


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[2:])
def test_emu_mem_balance_and_failure_sweep(mem, index, oracle, family):
    aux = index + (oracle,)
    before, t0 = mem.live(), mem.total()
    lib, rc = create()
    assert rc == 0 and family(lib, aux) == 0
    lib.close()
    assert mem.live() == before                              # balance
    n = mem.total() - t0
    assert n > 4
    for k in range(n):                                       # failure sweep: no k is skipped
        mem.fail_after(k)
        lib, rc = create()
        if lib is None:
            assert rc == E_NOMEM, k
            lib, rc = create()
            assert rc == 0, k
        else:
            assert family(lib, aux) == E_NOMEM, k
            assert lib.last_error(), k
        mem.fail_after(-1)
        assert family(lib, aux) == 0, (k, lib.last_error())
        lib.close()
        assert mem.live() == before, k


def m_run(md):
    try:
        got = md.mstream_compress(TEXT, 1, chunk=400, max_chunk=512)
    except BzxError as e:
        return e.code
    assert got == bz2.compress(TEXT, 1)
    return 0


def m_create():
    try:
        return MDev([0], EMU_PATH), 0
    except BzxError as e:
        return None, e.code


def test_emu_mem_mstream_one_entry(mem):
    """The same two checks for bzx_mctx / bzx_mstream with one entry."""
    before, t0 = mem.live(), mem.total()
    md, rc = m_create()
    assert rc == 0 and m_run(md) == 0
    md.close()
    assert mem.live() == before
    n = mem.total() - t0
    assert n > 4
    for k in range(n):
        mem.fail_after(k)
        md, rc = m_create()
        if md is None:
            assert rc == E_NOMEM, k
            md, rc = m_create()
            assert rc == 0, k
        else:
            assert m_run(md) == E_NOMEM, k
            assert md.last_error(), k
        mem.fail_after(-1)
        assert m_run(md) == 0, (k, md.last_error())
        md.close()
        assert mem.live() == before, k
