"""The set of bytes in use and the rank histogram of the MTF stage (bzx_mtf.hip) on whole small blocks.

The set is that of the block the BWT stage sorted -- the RLE1 image, not the raw input: run-length bytes join it.  The
split kernel of the bucket sorter and the MTF kernel each work it out for themselves (the split kernel keeps its copy
in LDS; nothing is handed from one stage to the other), so these inputs hold for both: one byte value, the two values
0 and 255, all 256, run-length bytes that the raw input does not contain, an exactly periodic block that the split
kernel refuses and the general sorter takes.  Each goes through bzx_compress_block and the one-block stream built from
its image is held against python's bz2, through the emulator (-m "not gpu") and on the device (-m gpu).

The zero-run pass counts RUNA, RUNB and rank 1 in registers and every deeper rank with an LDS atomic: last columns
through bzx_stage_mtf alone (no BWT stage) in which every head has rank 2 (more heads than one tile of 8,192, the
atomics all on one address), whose heads sit on the ranks 5 and 6, and whose ranks are spread over 1 to 9, against
the oracle.  Everything is equality."""
import bz2
import os
import random
import subprocess

import pytest

from bzx_ctypes import EMU_PATH, ROOT, BzxLib

_cache = {}


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = BzxLib(EMU_PATH)
    yield lib
    lib.close()


def _text(n, seed):
    rnd = random.Random(seed)
    words = [bytes(rnd.choices(b"etaoinshrdlucmfw", k=rnd.randint(2, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def _with_runs(n, run, seed):
    """Text with `run` (of a byte the text does not use) spliced in about every 60 bytes, n bytes or a little more."""
    rnd = random.Random(seed)
    t, out, i = _text(n, seed), bytearray(), 0
    while len(out) < n:
        step = rnd.randint(20, 100)
        out += t[i:i + step] + run
        i += step
    return bytes(out)                                   # (ends on a whole run)


RAW = {
    "one_value": lambda: b"q" * (255 * 40),                              # RLE1: 'qqqq' and the count byte 251
    "one_value_short_runs": lambda: b"q" * 4 * 1000 + b"q" * 3,        # ends on a run without a count byte
    "values_0_255": lambda: bytes(random.Random(1).choices((0, 255), k=5000)),
    "all_256": lambda: bytes(range(256)) * 2 + bytes(random.Random(2).choices(range(256), k=3600)),
    "runs_of_7": lambda: _with_runs(5000, b"a" * 7, 3),               # count byte 3: not a byte of the raw input
    "count_is_unused_value": lambda: _with_runs(8000, b"z" * 204, 4),  # count byte 200, in use nowhere else
    "count_is_used_value": lambda: _with_runs(8000, b"z" * (4 + ord("t")), 5),      # count byte 't': the set stays
    "periodic": lambda: b"ab" * 2000,
}


def _block(oracle, name):
    """(raw input, its one RLE1 block, CRC, libbz2's stream)."""
    if name not in _cache:
        raw = RAW[name]()
        assert 4000 <= len(raw) <= 40000
        (blk, crc), = oracle.split_rle1(raw, 9)
        _cache[name] = (raw, blk, crc, bz2.compress(raw, 9))
    return _cache[name]


def _one_block_stream(image, pad, crc):
    """'BZh9', the block image without its pad bits, the end-of-stream marker and the combined CRC of one block."""
    bits = len(image) * 8 - pad + 32 + 80
    v = (((int.from_bytes(b"BZh9" + image, "big") >> pad) << 48 | 0x177245385090) << 32 | crc) << (-bits % 8)
    return v.to_bytes((bits + 7) // 8, "big")


def _check_block(lib, oracle, name):
    raw, blk, crc, want = _block(oracle, name)
    image, pad = lib.compress_block(blk, crc)
    assert _one_block_stream(image, pad, crc) == want


COLUMNS = {
    "all_rank_2": lambda: b"abc" * 2800,                                 # 8,400 heads: crosses a tile of 8,192
    "ranks_5_and_6": lambda: b"abcdef" * 600 + b"abcdefg" * 600,        # a cycle of k symbols: every head has rank k - 1
    "ranks_1_to_9": lambda: bytes(random.Random(8).choices(range(10), k=6000)),
}


def _check_column(lib, oracle, name):
    if ("col", name) not in _cache:
        L = COLUMNS[name]()
        _cache["col", name] = (L, tuple(oracle.mtf(L))[:3])
    L, want = _cache["col", name]
    got = lib.stage_mtf(L)
    assert (list(got[0]), list(got[1]), bytes(got[2])) == (list(want[0]), list(want[1]), bytes(want[2]))


def test_inputs_are_what_their_names_say(oracle):
    """The RLE1 blocks hold the run-length bytes the names promise; every head of all_rank_2 but the first three has
    rank 2, and ranks_5_and_6 has heads on both ranks."""
    raw, blk, _, _ = _block(oracle, "one_value")
    assert set(raw) == {ord("q")} and set(blk) == {ord("q"), 251}
    raw, blk, _, _ = _block(oracle, "runs_of_7")
    assert 3 not in set(raw) and 3 in set(blk)
    raw, blk, _, _ = _block(oracle, "count_is_unused_value")
    assert 200 not in set(raw) and 200 in set(blk)
    raw, blk, _, _ = _block(oracle, "count_is_used_value")
    assert set(raw) == set(blk) and len(blk) < len(raw)
    assert set(_block(oracle, "values_0_255")[0]) == {0, 255}
    assert len(set(_block(oracle, "all_256")[1])) == 256
    mtfv, freq = oracle.mtf(COLUMNS["all_rank_2"]())[:2]
    assert freq[3] >= 8390 and len(mtfv) > 8192
    freq = oracle.mtf(COLUMNS["ranks_5_and_6"]())[1]
    assert freq[6] > 3000 and freq[7] > 3000


@pytest.mark.parametrize("name", list(RAW))
def test_emu_block(emu, oracle, name):
    _check_block(emu, oracle, name)


@pytest.mark.parametrize("name", list(COLUMNS))
def test_emu_column(emu, oracle, name):
    _check_column(emu, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RAW))
def test_gpu_block(bzx, oracle, name):
    _check_block(bzx, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(COLUMNS))
def test_gpu_column(bzx, oracle, name):
    _check_column(bzx, oracle, name)
