"""The per-table symbol frequencies of the Huffman stage (bzx_huff.hip) on the streams of tests/huff_count_cases.py.  The
kernel counts a group's low symbols (RUNA, RUNB, the first ranks) in packed register fields and adds them with a few
wide LDS atomics, and counts every symbol above that range with an atomic of its own: the cases sit on the edges of that
split -- an alphabet that ends inside the packed range, groups of one symbol on either side of its boundary, streams
without a packed symbol, short last groups (their unused places are padded, not tested for), ties between tables.

Harness and rule are those of test_huffman_edges.py: bzx_stage_huffman against the oracle's table optimisation and
bzx_stage_encode against bzo_encode_block, every case through the emulator (-m "not gpu") and on the device (-m gpu).
Everything is equality."""
import os
import subprocess

import pytest

import huff_cases as H
import huff_count_cases as K
from bzx_ctypes import EMU_PATH, ROOT, BzxLib

NAMES = list(K.CASES)
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
        mtfv, alpha = K.CASES[name]()
        assert mtfv[-1] == alpha - 1 and mtfv.count(alpha - 1) == 1 and max(mtfv) < alpha and len(mtfv) <= 30001
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


def test_cases_are_what_their_names_say():
    """Sizes, alphabets and symbol ranges the cases are named after; the tie case has ties in the first pass."""
    P = K.PACKED
    size = {name: len(K.CASES[name]()[0]) for name in NAMES}
    syms = {name: set(K.CASES[name]()[0][:-1]) for name in ("a3_even", "above_only", "boundary_pair", "solid_a11",
                                                            "solid_last_packed", "solid_first_unpacked", "tie_packed")}
    assert syms["a3_even"] == {0, 1} and K.CASES["a3_even"]()[1] == 3 < P
    assert min(syms["above_only"]) == P and syms["boundary_pair"] == {P - 1, P}
    assert syms["solid_a11"] == set(range(P + 1))
    assert syms["solid_last_packed"] == {P - 1} and syms["solid_first_unpacked"] == {P}
    assert size["a3_eob_alone"] % K.G == 1 and size["last_1"] % K.G == 1 and size["last_49"] % K.G == 49
    assert [size[f"runa_{n}"] for n in (199, 200, 599, 2399, 2400)] == [199, 200, 599, 2399, 2400]
    for n in (199, 200, 599, 2399, 2400):
        mtfv = K.CASES[f"runa_{n}"]()[0]
        assert 0.85 < mtfv.count(0) / n < 0.95
    assert (size["few_groups"] + 49) // 50 < 512 and (size["sel_513"] + 49) // 50 == 513
    mtfv, alpha = K.CASES["tie_packed"]()
    assert max(mtfv) < P and len(mtfv) >= 2400
    assert K.first_pass_ties(mtfv, alpha) >= 100
    for name in ("solid_a11", "solid_a258", "solid_last_packed", "solid_first_unpacked"):
        mtfv = K.CASES[name]()[0]
        assert all(len(set(mtfv[g:g + K.G])) == 1 for g in range(0, len(mtfv) - 1, K.G)), name


@pytest.mark.parametrize("name", NAMES)
def test_emu_case(emu, oracle, name):
    _check_case(emu, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(bzx, oracle, name):
    _check_case(bzx, oracle, name)
