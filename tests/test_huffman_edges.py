"""The Huffman stage (bzx_huff.hip) and the emitter (bzx_emit.hip) on symbol streams no ordinary input produces
(tests/huff_cases.py): code lengths that libbz2's limiter has to bring down to 17 bits by halving the weights, 16- and
17-bit codes in the payload, the table-count thresholds, selector counts around the 512-lane chunks of the selector MTF
and the emitter's 512-group tiles, the largest streams, empty initial partitions, ties.

bzx_stage_huffman is held against the oracle's table optimisation, bzx_stage_encode (Huffman stage + emit stage of one
block over a given symbol stream) against bzo_encode_block in image, pad bits, selector MTF, section sizes and total:
through the emulator (-m "not gpu", every case) and on the device (-m gpu, every case).  Everything is equality.

One byte input reaches the limiter from the BWT on: 899,000 bytes of 20 values with weights 2^-i, taken as one block
(handed to the RLE1 splitter first it becomes two blocks and the first stays at a depth of exactly 17).  Its block goes
through the emulated stages from its symbol stream on, and on the device through bzx_compress_block; libbz2 decodes
the image.  The same generator at 860,000 bytes is one block after RLE1 as well and
retries there, so that input goes through the stream forms: the oracle and bzx_compress_buffer against live
bz2.compress, and back through bzx_decompress_buffer.  The oracle's limiter is also held against
BZ2_hbMakeCodeLengths of the live libbz2 directly."""
import bz2
import os
import random
import subprocess

import pytest

import huff_cases as H
from bz2_writer import rle1_decode
from bzx_ctypes import EMU_PATH, ROOT, BzxLib

NAMES = list(H.CASES)
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


def _case(oracle, name):
    """(stream, alphabet, frequencies, symbol map, origPtr, CRC, the oracle's tables, the oracle's block): built once."""
    if name not in _cache:
        mtfv, alpha = H.CASES[name]()
        assert mtfv[-1] == alpha - 1 and mtfv.count(alpha - 1) == 1 and max(mtfv) < alpha
        freq, in_use = H.freq_of(mtfv), H.in_use_for(alpha)
        k = NAMES.index(name) + 1
        orig, crc = (k * 7919) % len(mtfv), (k * 0x9E3779B9) & 0xFFFFFFFF
        _cache[name] = (mtfv, alpha, freq, in_use, orig, crc, oracle.huff(mtfv, freq, alpha),
                        oracle.encode_block(mtfv, freq, in_use, orig, crc))
    return _cache[name]


def _check_case(lib, oracle, name):
    mtfv, alpha, freq, in_use, orig, crc, want_huff, want_enc = _case(oracle, name)
    assert lib.stage_huffman(mtfv, freq, alpha) == want_huff
    got = lib.stage_encode(mtfv, freq, in_use, orig, crc)
    assert got[3] == want_enc[3]                    # tables, selectors, the four section sizes, total bits
    assert got[2] == want_enc[2]                    # selector MTF
    assert got[1] == want_enc[1]                    # pad bits
    assert got[0] == want_enc[0]                    # the image


def _seed4(oracle):
    """The byte input of the module text, taken as ONE block (the bytes are the RLE1 image, as bzx_compress_block takes
    them; split by RLE1 instead, its first block stays one level short of the limiter): (data, the bytes that image
    stands for, their CRC, the block's origPtr, symbols, frequencies, symbol map and alphabet, the oracle's block)."""
    if "seed4" not in _cache:
        data = bytes(random.Random(4).choices(range(20), weights=[2.0 ** -i for i in range(1, 21)], k=899000))
        raw = bytes(rle1_decode(data))
        crc = oracle.crc32(raw)
        L, orig = oracle.bwt(data)
        mtfv, freq, in_use, niu = oracle.mtf(L)
        _cache["seed4"] = (data, raw, crc, orig, mtfv, freq, in_use, niu + 2, oracle.compress_block(data, crc))
    return _cache["seed4"]


def _stream4(oracle):
    """860,000 bytes of the same generator: ONE block after RLE1 too, and it retries: (data, libbz2's stream)."""
    if "stream4" not in _cache:
        data = bytes(random.Random(4).choices(range(20), weights=[2.0 ** -i for i in range(1, 21)], k=860000))
        (blk, _crc), = oracle.split_rle1(data, 9)
        mtfv, _freq, _in_use, niu = oracle.mtf(oracle.bwt(blk)[0])
        halvings, longest, depth = H.certify(oracle, mtfv, niu + 2)
        assert halvings >= 1 and depth > 17 and longest == 17
        _cache["stream4"] = (data, bz2.compress(data, 9))
    return _cache["stream4"]


def _one_block_stream(image, pad, crc):
    """'BZh9', the block image without its pad bits, the end-of-stream marker and the combined CRC of one block."""
    bits = len(image) * 8 - pad + 32 + 80
    v = (((int.from_bytes(b"BZh9" + image, "big") >> pad) << 48 | 0x177245385090) << 32 | crc) << (-bits % 8)
    return v.to_bytes((bits + 7) // 8, "big")


def _libbz2_code_lengths(freq, alpha, max_len=17):
    """BZ2_hbMakeCodeLengths of the libbz2 that python's bz2 module runs on."""
    import ctypes as C
    import ctypes.util
    lib = C.CDLL(ctypes.util.find_library("bz2"))
    lib.BZ2_bzlibVersion.restype = C.c_char_p
    assert lib.BZ2_bzlibVersion().startswith(b"1.0.")
    ln = (C.c_uint8 * 258)()
    f = (C.c_int32 * 258)(*(list(freq) + [0] * (258 - len(freq))))
    lib.BZ2_hbMakeCodeLengths.restype = None
    lib.BZ2_hbMakeCodeLengths.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.BZ2_hbMakeCodeLengths(ln, f, alpha, max_len)
    return list(ln[:alpha])


# ---------------------------------------------------------------- CPU

def test_retry_cases_are_certified(oracle):
    """From the oracle's final selectors: every retry case halves the weights of some table at least once, one of them
    twice or more, and each ends with a 17-bit code; fib25 has a 17-bit code that needed no halving; heavy_groups has a
    group of 850 payload bits.  (A generator
    changed later cannot quietly turn these into ordinary cases.)"""
    most = 0
    for name in H.RETRY:
        mtfv, alpha = _case(oracle, name)[:2]
        halvings, longest, depth = H.certify(oracle, mtfv, alpha)
        assert halvings >= 1 and depth > 17 and longest == 17, (name, halvings, longest, depth)
        most = max(most, halvings)
    assert most >= 2
    for name in H.LONG_NO_RETRY:
        mtfv, alpha = _case(oracle, name)[:2]
        assert H.certify(oracle, mtfv, alpha) == (0, 17, 17), name
    for name in H.HEAVY:                            # a group of fifty 17-bit codes: the most a group's payload can be
        mtfv, alpha = _case(oracle, name)[:2]
        assert max(H.group_payloads(oracle, mtfv, alpha)) == 850, name


def test_case_list_covers_the_edges():
    """The sizes the cases are named after are the sizes they have."""
    sizes = {name: len(H.CASES[name]()[0]) for name in NAMES if name.startswith(("thr_", "tile_", "max_"))}
    assert {sizes[f"thr_{n}_a{a}"] for n in H.THRESHOLDS for a in (4, 258)} == set(H.THRESHOLDS)
    for ns in H.TILE_SELECTORS:
        for last in (50, 1, 49):
            n = sizes[f"tile_{ns}_last{last}"]
            assert (n + 49) // 50 == ns and n % 50 == last % 50
    assert sizes["max_flat"] == sizes["max_900001"] == 900001 and sizes["max_900000"] == 900000


def test_oracle_limiter_is_libbz2s(oracle):
    """bzo_make_code_lengths against the function libbz2 itself exports, at the limit of 17: on the frequencies of
    every table of the final pass of the retry cases and of the byte input's block, and on Fibonacci and power-of-two
    frequencies of 19 to 258 symbols that need several halvings."""
    vectors = []
    for name in list(H.RETRY) + list(H.LONG_NO_RETRY):
        mtfv, alpha = _case(oracle, name)[:2]
        vectors += [(rf, alpha) for rf, _ in H.final_tables(oracle, mtfv, alpha)]
    mtfv, alpha = _seed4(oracle)[4], _seed4(oracle)[7]
    vectors += [(rf, alpha) for rf, _ in H.final_tables(oracle, mtfv, alpha)]
    rnd = random.Random(17)
    for alpha in (19, 20, 24, 30, 31, 40, 64, 65, 129, 258):
        fib, a, b = [], 1, 1
        for _ in range(min(alpha, 30)):
            fib.append(a)
            a, b = b, a + b
        for base in (fib, [1 << s for s in range(min(alpha, 21))]):
            f = (base + [0, 1, 2, 3] * 65)[:alpha]
            assert sum(f) < 1 << 22                 # (weights are frequencies << 8 in 32 bits; a block has 900,001 symbols)
            vectors.append((f, alpha))
            g = f[:]
            rnd.shuffle(g)
            vectors.append((g, alpha))
    most = 0
    for f, alpha in vectors:
        assert oracle.make_code_lengths(f, alpha, 17) == _libbz2_code_lengths(f, alpha), (alpha, f)
        most = max(most, H.max_depth_and_halvings(oracle, f, alpha)[1])
    assert most >= 4


def test_byte_input_retries_and_libbz2_reads_it(oracle):
    """The byte input: as one block it retries (one table of its final pass is 18 deep without the limit) and ends
    with 17-bit codes, libbz2 decodes the oracle's image of that block, and the oracle's stream of the input is
    libbz2's."""
    data, raw, crc, orig, mtfv, freq, in_use, alpha, want = _seed4(oracle)
    halvings, longest, depth = H.certify(oracle, mtfv, alpha)
    assert halvings >= 1 and depth > 17 and longest == 17
    assert bz2.decompress(_one_block_stream(want[0], want[1], crc)) == raw
    assert oracle.compress(data, 9)[0] == bz2.compress(data, 9)


def test_oracle_stream_that_retries_is_libbz2s(oracle):
    """The stream form: an input that is one block after RLE1 and retries there (_stream4 asserts both); the oracle's
    stream is live libbz2's."""
    data, z = _stream4(oracle)
    assert oracle.compress(data, 9) == (z, 1)


@pytest.mark.parametrize("name", NAMES)
def test_emu_case(emu, oracle, name):
    _check_case(emu, oracle, name)


def test_emu_retry_block_from_its_symbols(emu, oracle):
    """The block of the byte input from the MTF stage's output on: the emulated Huffman and emit stages give the
    image the oracle's compress_block gives."""
    data, raw, crc, orig, mtfv, freq, in_use, alpha, want = _seed4(oracle)
    assert emu.stage_huffman(mtfv, freq, alpha) == oracle.huff(mtfv, freq, alpha)
    assert emu.stage_encode(mtfv, freq, in_use, orig, crc)[:2] == want


def test_emu_stage_encode_refusals(emu, oracle):
    """bzx_stage_encode's argument checks: those of bzx_stage_huffman, a symbol outside the alphabet, origPtr beyond
    24 bits; a cap too small reports the bytes needed."""
    import ctypes as C
    from bzx_ctypes import BzxError
    mtfv, alpha, freq, in_use, orig, crc, _, want = _case(oracle, "thr_51_a4")
    for bad in (dict(mtfv=[]), dict(in_use=bytes(256)), dict(orig=1 << 24),
                dict(mtfv=list(mtfv[:-1]) + [alpha])):
        a = dict(mtfv=mtfv, in_use=in_use, orig=orig)
        a.update(bad)
        with pytest.raises(BzxError) as e:
            emu.stage_encode(a["mtfv"], freq, a["in_use"], a["orig"], crc)
        assert e.value.code == -2, bad
    arr = (C.c_uint16 * len(mtfv))(*mtfv)
    f = (C.c_uint32 * 258)(*freq)
    out, ol, pad = C.create_string_buffer(8), C.c_size_t(), C.c_uint8()
    from bzx_ctypes import BzxBlockInfo
    rc = emu.lib.bzx_stage_encode(emu.ctx, arr, len(mtfv), f, in_use, orig, crc, out, 8, C.byref(ol), C.byref(pad),
                                  (C.c_uint8 * 18002)(), C.byref(BzxBlockInfo()))
    assert rc == -4 and ol.value == len(want[0])
    assert emu.stage_encode(mtfv, freq, in_use, orig, crc) == want


# ---------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(bzx, oracle, name):
    _check_case(bzx, oracle, name)


@pytest.mark.gpu
def test_gpu_retry_input_whole_pipeline(bzx, oracle):
    """The byte input that retries, through everything: as one block through bzx_compress_block against the oracle
    (libbz2 decodes the device's image), the stages from its symbol stream on, the buffer through bzx_compress_buffer
    against live libbz2 and the oracle against libbz2, and back through bzx_decompress_buffer."""
    data, raw, crc, orig, mtfv, freq, in_use, alpha, want = _seed4(oracle)
    halvings, longest, depth = H.certify(oracle, mtfv, alpha)
    assert halvings >= 1 and depth > 17 and longest == 17
    got = bzx.compress_block(data, crc)
    assert got == want
    z1 = _one_block_stream(got[0], got[1], crc)
    assert bz2.decompress(z1) == raw
    assert bzx.stage_huffman(mtfv, freq, alpha) == oracle.huff(mtfv, freq, alpha)
    assert bzx.stage_encode(mtfv, freq, in_use, orig, crc)[:2] == want
    z = bz2.compress(data, 9)
    assert oracle.compress(data, 9)[0] == z
    assert bzx.compress_buffer(data, 9) == z
    assert bzx.decompress_buffer(z) == data
    assert bzx.decompress_buffer(z1) == raw         # 17-bit codes from a limited tree through the device's decoder


@pytest.mark.gpu
def test_gpu_stream_that_retries(bzx, oracle):
    """The stream form on the device: an input that is one block after the device's RLE1 split and retries there, through
    bzx_compress_buffer (16- and 17-bit codes of a limited tree emitted at the stream's bit offset 32) against live
    libbz2 and the oracle, and libbz2's stream back through bzx_decompress_buffer."""
    data, z = _stream4(oracle)
    assert oracle.compress(data, 9) == (z, 1)
    assert [(len(b), c) for b, c in bzx.split_rle1(data, 9)] == [(len(b), c) for b, c in oracle.split_rle1(data, 9)]
    assert bzx.compress_buffer(data, 9) == z
    assert bzx.decompress_buffer(z) == data
