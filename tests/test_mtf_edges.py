"""The MTF and zero-run stage (bzx_mtf.hip) on last columns no BWT of ordinary input produces (tests/mtf_cases.py):
every ranking variant and width of the recency code, both placements of the recency lists, chunk counts around the
waves of the start lists, symbols that appear late, the tile edges of pass 1 and pass 6, the staging bound of pass 6,
a symbol left waiting at a tile start and at EOB, zero runs of 1 to 19 digits.

mtf_cases.shape() mirrors the kernel's arithmetic, and test_case_list_covers_the_edges proves from it that the cases
reach what they are named after.  A plain Python model of the stage (and its inverse) is held against the oracle on
every case: that licenses the oracle, pinned to libbz2 through real streams only, as the expected value here.
bzx_stage_mtf is then held against the oracle through the emulator (-m "not gpu", every case) and on the device
(-m gpu, every case), on a fresh context, behind a 900,000-byte block on the same context, and back to back.
Everything is equality.  Symbol streams are compared as the bytes of their uint16 arrays."""
import ctypes as C
import os
import subprocess
from array import array

import pytest

import mtf_cases as M
from bzx_ctypes import EMU_PATH, ROOT, BzxLib

NAMES = list(M.CASES)
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


def _column(name):
    if ("L", name) not in _cache:
        L = M.CASES[name]()
        assert isinstance(L, bytes) and 1 <= len(L) <= M.MAX_BLOCK, name
        _cache["L", name] = L
    return _cache["L", name]


def _reference(name):
    """mtf_reference of the case, its symbols as bytes: built once."""
    if ("ref", name) not in _cache:
        sym, freq, in_use = M.mtf_reference(_column(name))
        _cache["ref", name] = (sym.tobytes(), freq, in_use)
    return _cache["ref", name]


def _shape(name):
    if ("shape", name) not in _cache:
        _cache["shape", name] = M.shape(_column(name), _symbols(_reference(name)[0]))
    return _cache["shape", name]


def _symbols(raw):
    a = array("H")
    a.frombytes(raw)
    return a


def _oracle_mtf(oracle, L):
    """Oracle.mtf without the lists: (symbols as bytes, freq, in_use)."""
    n = len(L)
    mtfv = (C.c_uint16 * (n + 2))()
    freq = (C.c_int32 * 258)()
    in_use = (C.c_uint8 * 256)()
    niu = C.c_int32()
    oracle.lib.bzo_mtf_rle2.restype = C.c_int32
    m = oracle.lib.bzo_mtf_rle2(L, n, mtfv, freq, in_use, C.byref(niu))
    assert niu.value == sum(in_use)
    return C.string_at(mtfv, 2 * m), list(freq), bytes(in_use)


def _stage_mtf(lib, L):
    """BzxLib.stage_mtf without the lists: (symbols as bytes, freq, in_use).  The output arrays start out as 0xA5 so that
    a symbol the stage never wrote cannot pass for a RUNA."""
    n = len(L)
    mtfv = (C.c_uint16 * (n + 2))()
    C.memset(mtfv, 0xA5, 2 * (n + 2))
    n_mtf = C.c_uint32()
    freq = (C.c_uint32 * 258)()
    in_use = (C.c_uint8 * 256)()
    lib._check(lib.lib.bzx_stage_mtf(lib.ctx, L, n, mtfv, C.byref(n_mtf), freq, in_use))
    return C.string_at(mtfv, 2 * n_mtf.value), list(freq), bytes(in_use)


def _want(oracle, name):
    if ("want", name) not in _cache:
        _cache["want", name] = _oracle_mtf(oracle, _column(name))
    return _cache["want", name]


def _dirty_sequence(lib, oracle, again):
    """The 900,000-byte 256-symbol column, then the smallest cases on the same context: heads, positions, lists and
    symbols the big block left behind must not show."""
    assert _stage_mtf(lib, _column(M.BIG)) == _want(oracle, M.BIG)
    for name in M.AFTER_BIG:
        assert _stage_mtf(lib, _column(name)) == _want(oracle, name), name
    if again:
        assert _stage_mtf(lib, _column(M.BIG)) == _want(oracle, M.BIG)


# ---------------------------------------------------------------- CPU

def test_case_list_covers_the_edges():
    """From shape() over CASES: every path below is reached by a named case.  An edit of the list or of a kernel
    constant (mirrored in mtf_cases.py) that loses one fails here; so does the removal of any one group of cases."""
    S = {name: _shape(name) for name in NAMES}
    sh = list(S.values())
    assert sum(len(g) for g in M.GROUPS.values()) == len(NAMES)
    assert sum(1 for s in sh if s.n == M.MAX_BLOCK) <= 13

    # ranking variants, each with the deepest rank the alphabet allows; widths; placement of the recency lists
    for variant in ("regs1", "regs2", "regs3", "regs4", "lds"):
        assert any(s.variant == variant and s.n_in_use > 1 and s.deepest_rank == s.n_in_use - 1 for s in sh), variant
    for lo, hi in ((2, 8), (9, 16), (17, 24), (25, 32), (33, 64), (65, 128), (129, 256)):   # both ends of every range
        assert {lo, hi} <= {s.n_in_use for s in sh}, (lo, hi)
    assert {s.nw for s in sh} == {1, 2, 4}
    assert {s.rec_in_lds for s in sh} == {True, False}
    # the four-word walk reads past the last word of a list whose stride is not 1 + a multiple of 32 bytes
    assert any(s.variant == "lds" and (s.stride // 8 - 1) % 4 and s.deepest_rank == s.n_in_use - 1 for s in sh)
    assert any(73 <= s.n_in_use <= 80 and s.deepest_rank == s.n_in_use - 1 for s in sh)
    # as many heads as a block can have, P[nh] the last word in use
    for nw in (1, 2, 4):
        assert any(s.nw == nw and s.nh == M.MAX_BLOCK for s in sh), nw

    # chunk counts: one chunk, one wave, one chunk into the second wave, all of them (two- and 256-symbol lists),
    # the last chunk of all with a single head, the first chunk size of 32
    for small in (True, False):
        mine = [s for s in sh if (s.n_in_use <= 8) == small and (small or s.n_in_use == 256)]
        assert ({1, 64, 65} if small else {64, 65}) <= {s.nch_used for s in mine}, small
        assert any(s.nch_used == s.nch and s.csz == 16 and s.nh == 16 * s.nch for s in mine), small
        assert any(s.nch_used == s.nch and s.csz == 16 and s.nh == 16 * (s.nch - 1) + 1 for s in mine), small
        assert any(s.csz == 32 and s.nh == 16 * s.nch + 1 for s in mine), small
    assert M.chunks_available(2) == 1024 and M.chunks_available(256) == 558

    # start lists: symbols that first appear behind the first wave (small and large alphabet), group lists passed over
    assert any(s.late_symbols >= 3 and s.nw == 1 for s in sh)
    assert any(s.late_symbols >= 250 and s.nw == 4 for s in sh)
    assert any(s.skipped_groups >= 1 and s.nw == 4 for s in sh)

    # pass 1: more than one tile and a ragged end; n at a tile - 1, a tile, a tile + 1
    assert any(s.tiles1 > 1 and s.n % M.TILE1 for s in sh)
    assert {M.TILE1 - 1, M.TILE1, M.TILE1 + 1, M.TILE1 + M.MTF_E - 1, M.TILE1 + M.MTF_E, M.TILE1 + M.MTF_E + 1} \
        <= {s.n for s in sh}

    # pass 6: a symbol waiting at a tile start; tiles that all emit odd counts, with an odd and an even total; the
    # symbol still waiting at the third tile; the staging bound, alone and with a symbol waiting behind it
    assert any(s.tiles6 >= 2 and s.odd_tile_start for s in sh)
    assert {s.odd_before_eob for s in sh} == {True, False}
    all_odd = [s for s in sh if s.tiles6 >= 3 and all(c & 1 for c in s.tile_counts)]
    assert {s.odd_before_eob for s in all_odd} == {True, False}
    assert any(s.tiles6 == 3 and s.tile_counts[0] & 1 and not s.tile_counts[1] & 1 for s in sh)
    assert any(s.max_staged >= 63214 for s in sh)
    assert any(s.tile_counts[0] >= 63200 and s.tile_counts[0] & 1 and s.tiles6 >= 2 for s in sh)
    assert all(s.max_staged <= 63219 + 1 for s in sh)              # the bound bzx_mtf.hip derives, and a pending symbol

    # first head; zero runs of every digit count; a full-size block whose heads spread over every rank of 256 symbols
    assert {s.first_rank0 for s in sh} == {True, False}
    assert any(s.first_rank0 and s.nh > 1 for s in sh)
    assert set().union(*(s.run_digits for s in sh)) >= set(range(1, 20))
    assert any(s.n == M.MAX_BLOCK and s.n_in_use == 256 and s.spread_ranks == 255 for s in sh)
    assert {S[name].nh for name in ("n1", "one_run_900000")} == {1}


def test_reference_agrees_with_oracle(oracle):
    """The plain model and the oracle agree on every case in symbols, histogram and bytes in use, and the model's
    inverse takes the oracle's symbols back to the column."""
    for name in NAMES:
        want = _want(oracle, name)
        assert _reference(name) == want, name
        assert M.mtf_inverse(_symbols(want[0]), want[2]) == _column(name), name


@pytest.mark.parametrize("name", NAMES)
def test_emu_case(emu, oracle, name):
    assert _stage_mtf(emu, _column(name)) == _want(oracle, name)


def test_emu_dirty_context(emu, oracle):
    _dirty_sequence(emu, oracle, again=False)


# ---------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(bzx, oracle, name):
    got = _stage_mtf(bzx, _column(name))
    assert got == _want(oracle, name)
    assert M.mtf_inverse(_symbols(got[0]), got[2]) == _column(name)        # (this one owes the oracle nothing)


@pytest.mark.gpu
def test_gpu_dirty_context(bzx, oracle):
    _dirty_sequence(bzx, oracle, again=True)


@pytest.mark.gpu
def test_gpu_cases_back_to_back(bzx, oracle):
    """Every case, then every case in reverse order, on the one context: nothing a block leaves behind in the slabs
    (heads, positions, recency lists in the symbol slab) reaches the next, whatever came before it."""
    for name in NAMES + NAMES[::-1]:
        assert _stage_mtf(bzx, _column(name)) == _want(oracle, name), name
