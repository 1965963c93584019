"""The emit stage at the seams of its work items (bzx_emit.hip): a block's payload is cut into tiles of T 50-symbol
groups, I consecutive tiles of a block make one work item, a tile's bits are packed in an LDS staging area of S bits and
copied out by the whole workgroup, the first and last word of a tile merged with atomicOr.  T, I and S come from the
build under test (bzx_emit_geometry); the streams are those of emit_tile_cases.py.

Harness and rule are those of test_huffman_edges.py: bzx_stage_encode against bzo_encode_block -- image, pad bits,
selector MTF, section sizes, total -- every case through the emulator (-m "not gpu") and on the device (-m gpu).  On
the device also one batched call over inputs of very different tile counts (its level 1 form through the emulator too)
and one five-block stream, against bz2.compress.  Everything is equality.  There is no second store path to test: S holds the largest tile there can be (asserted below)."""
import bz2
import os
import subprocess

import pytest

import emit_tile_cases as E
import huff_cases as H
from bzx_batch_ctypes import BatchLib
from bzx_ctypes import EMU_PATH, ROOT

SEAMS = [(k, last) for k in range(E.N_SEAMS) for last in E.LASTS]
SEEDS = list(range(len(E.SEEDED)))
_cache = {}


def _build_emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])


@pytest.fixture(scope="module")
def emu():
    _build_emu()
    lib = BatchLib(EMU_PATH)
    yield lib
    lib.close()


def _case(oracle, key, build):
    """(stream, alphabet, frequencies, symbol map, origPtr, CRC, the oracle's block): built once per stream."""
    if key not in _cache:
        mtfv, alpha = build()
        assert mtfv[-1] == alpha - 1 and mtfv.count(alpha - 1) == 1 and max(mtfv) < alpha
        freq, in_use = H.freq_of(mtfv), H.in_use_for(alpha)
        k = len(_cache) + 1
        orig, crc = (k * 7919) % len(mtfv), (k * 0x9E3779B9) & 0xFFFFFFFF
        _cache[key] = (mtfv, alpha, freq, in_use, orig, crc, oracle.encode_block(mtfv, freq, in_use, orig, crc))
    return _cache[key]


def _seam(oracle, T, I, k, last):
    c = _case(oracle, ("seam", T, I, k, last), lambda: E.seam_case(T, I, k, last))
    assert c[6][3][1] == E.seam_groups(T, I, k, last) and (len(c[0]) - 1) % E.G + 1 == last
    return c


def _seeded(oracle, T, k):
    return _case(oracle, ("seed", T, k), lambda: E.seeded_case(T, k))


def _check(lib, case):
    mtfv, alpha, freq, in_use, orig, crc, want = case
    got = lib.stage_encode(mtfv, freq, in_use, orig, crc)
    assert got[3] == want[3]                    # tables, selectors, the four section sizes, total bits
    assert got[2] == want[2]                    # selector MTF
    assert got[1] == want[1]                    # pad bits
    assert got[0] == want[0]                    # the image


def test_geometry_and_word_seams(emu, oracle):
    """The staging area holds the largest tile (T groups of fifty 17-bit codes), so every tile takes the one store path.
    Over the seam cases and the seeded ones, recomputed from the oracle's tables and selectors: the tiles start at every
    bit phase of a word, one ends exactly on a word boundary, one is shorter than a word."""
    T, I, S = E.geometry(emu.lib)
    assert T >= 64 and I >= 1 and S >= T * E.G * 17
    sel = E.seam_selectors(T, I)
    assert len(sel) == E.N_SEAMS and len(set(sel)) == E.N_SEAMS and min(sel) == 1 and max(sel) == E.MAX_SEL
    phases, on_boundary, short = set(), 0, 0
    cases = [_seam(oracle, T, I, k, last) for k, last in SEAMS] + [_seeded(oracle, T, k) for k in SEEDS]
    for mtfv, alpha, _, _, _, _, want in cases:
        spans = E.tile_spans(oracle, mtfv, alpha, T, want[3])
        assert len(spans) == (want[3][1] + T - 1) // T
        for start, bits in spans:
            phases.add(start % 32)
            on_boundary += (start + bits) % 32 == 0
            short += bits < 32
    assert phases == set(range(32))
    assert on_boundary >= 1 and short >= 1


@pytest.mark.parametrize("k,last", SEAMS)
def test_emu_seam(emu, oracle, k, last):
    T, I, _ = E.geometry(emu.lib)
    _check(emu, _seam(oracle, T, I, k, last))


@pytest.mark.parametrize("k", SEEDS)
def test_emu_seeded(emu, oracle, k):
    _check(emu, _seeded(oracle, E.geometry(emu.lib)[0], k))


@pytest.mark.gpu
@pytest.mark.parametrize("k,last", SEAMS)
def test_gpu_seam(bzx, oracle, k, last):
    T, I, _ = E.geometry(bzx.lib)
    _check(bzx, _seam(oracle, T, I, k, last))


@pytest.mark.gpu
@pytest.mark.parametrize("k", SEEDS)
def test_gpu_seeded(bzx, oracle, k):
    _check(bzx, _seeded(oracle, E.geometry(bzx.lib)[0], k))


def _mixed_inputs(oracle, level):
    """1 B, 60 B, about 2.6 KB and one full block of the level (100,000 * level - 19 bytes that RLE1 leaves alone): at
    level 9 one to 36 tiles."""
    if ("mixed", level) not in _cache:
        inputs = [b"q", oracle.synthtext(60, seed=3), oracle.synthtext(2600, seed=4),
                  oracle.synthtext(100000 * level - 19, seed=5)]
        _cache["mixed", level] = (inputs, [bz2.compress(x, level) for x in inputs])
    return _cache["mixed", level]


def test_emu_batch_of_very_different_blocks(emu, oracle):
    """(the emulator takes the level 1 form: its full block is a ninth of the device test's)"""
    inputs, want = _mixed_inputs(oracle, 1)
    assert emu.batch_buffer(inputs, 1) == want


@pytest.mark.gpu
def test_gpu_batch_of_very_different_blocks(oracle):
    inputs, want = _mixed_inputs(oracle, 9)
    lib = BatchLib()
    try:
        assert lib.batch_buffer(inputs, 9) == want
    finally:
        lib.close()


def _five_blocks(oracle):
    """About 450 KB of text at level 1: five blocks that start at whatever bit the block in front ends on."""
    if "five" not in _cache:
        data = oracle.synthtext(450_000, seed=6)
        want = bz2.compress(data, 1)
        assert oracle.compress(data, 1) == (want, 5)
        _cache["five"] = (data, want)
    return _cache["five"]


@pytest.mark.gpu
def test_gpu_stream_of_five_blocks(bzx, oracle):
    import torch
    data, want = _five_blocks(oracle)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
    d_out = torch.zeros(len(data) + len(data) // 50 + 4096, dtype=torch.uint8, device="cuda")
    n = bzx.compress_device(d_in.data_ptr(), len(data), 1, d_out.data_ptr(), d_out.numel())
    assert d_out[:n].cpu().numpy().tobytes() == want
