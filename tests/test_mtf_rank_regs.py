"""The register rank loop of bzx_mtf.hip (alphabets of at most 32 byte values: the MTF list in NR = ceil(n_in_use / 4)
32-bit registers) on the columns of tests/mtf_rank_cases.py: a hit in every byte of every register for every register
count, alphabets of high and scattered byte values, the one head of rank 0, short last groups of 16 heads, the order of
the list after deep hits, and a small alphabet behind a large one on the same context.

test_cases_reach_what_they_name proves from mtf_cases.shape() that the columns are what their names say.  bzx_stage_mtf
is held against the oracle's bzo_mtf_rle2 through the emulator (every case) and on the device (-m gpu, every case), each
case on a context of its own; symbols (as the bytes of their uint16 array), freq and in_use are compared for equality."""
import pytest

import mtf_cases as M
import mtf_rank_cases as R
from bzx_ctypes import EMU_PATH, LIB_PATH, BzxLib
from test_mtf_edges import _oracle_mtf, _stage_mtf, emu  # noqa: F401  (emu: the fixture that builds the emulator)

NAMES = list(R.CASES)
_cache = {}


def _column(name):
    if ("L", name) not in _cache:
        L = R.CASES[name]()
        assert isinstance(L, bytes) and 1 <= len(L) <= 41_000, name
        _cache["L", name] = L
    return _cache["L", name]


def _want(oracle, name):
    if ("want", name) not in _cache:
        _cache["want", name] = _oracle_mtf(oracle, _column(name))
    return _cache["want", name]


def _run_fresh(path, oracle, names):
    """The named cases one after the other on one new context."""
    lib = BzxLib(path, max_blocks=1)
    try:
        for name in names:
            assert _stage_mtf(lib, _column(name)) == _want(oracle, name), name
    finally:
        lib.close()


# ---------------------------------------------------------------- CPU

def test_cases_reach_what_they_name():
    S = {name: M.shape(_column(name)) for name in NAMES}
    for name, s in S.items():
        assert sorted(set(_column(name))) == R.ALPHABET[name], name
        assert s.n_in_use <= 32 and s.variant == "regs%d" % ((s.n_in_use + 7) // 8), name
        assert s.csz % 16 == 0 and s.nch_used == -(-s.nh // s.csz), name

    # every entry position: all the sizes, three kinds of alphabet, the deepest rank, more than one wave of chunks
    for n in R.SIZES:
        for kind in ("low", "high", "scat"):
            s = S[f"every_{kind}_{n}"]
            assert s.n_in_use == n and s.deepest_rank == n - 1 and not s.first_rank0, (kind, n)
            assert s.spread_ranks == n - 1 and s.nch_used > 2 * M.MTF_GROUP, (kind, n)
        assert min(R.ALPHABET[f"every_high_{n}"]) >= 0x80
        assert min(R.ALPHABET[f"every_scat_{n}"]) < 0x80 <= max(R.ALPHABET[f"every_scat_{n}"])
    # both register counts of every range, with and without padding in the last register
    for variant, counts in (("regs1", (1, 2)), ("regs2", (3, 4)), ("regs3", (5, 6)), ("regs4", (7, 8))):
        for nr in counts:
            mine = [n for n in R.SIZES if R.registers(n) == nr]
            assert mine and all(S[f"every_low_{n}"].variant == variant for n in mine), nr
        assert any(n % 4 for n in R.SIZES if R.registers(n) in counts) and any(n % 4 == 0 for n in R.SIZES if R.registers(n) in counts)

    # rank 0 at the first head, and only there
    for n in (5, 28):
        s = S[f"first0_{n}"]
        assert s.first_rank0 and s.n_in_use == n and s.deepest_rank == n - 1 and s.nh > 16
    assert not S["every_high_5"].first_rank0 and not S["every_scat_28"].first_rank0

    # chunk tails: chunks of 16 heads, the last one short by what the name says
    for n in (2, 28):
        for nh in R.TAIL_HEADS:
            s = S[f"tail_{n}_nh{nh}"]
            assert s.nh == nh and s.n_in_use == min(n, nh) and s.csz == 16 and s.nch_used == -(-nh // 16), (n, nh)
        assert {S[f"tail_{n}_nh{nh}"].nh % 16 for nh in R.TAIL_HEADS} == {0, 1, 15}
        assert {S[f"tail_{n}_nh{nh}"].nch_used for nh in R.TAIL_HEADS} == {1, 2, 3, 4}
        for nh in (31, 17):                               # two used chunks, the second shorter than csz
            s = S[f"tail_{n}_nh{nh}"]
            assert s.nch_used == 2 and 0 < s.nh - s.csz < s.csz
        s = S[f"tail_{n}_nh16401"]                        # two groups of 16 per chunk, the last chunk with one and a head
        assert s.n_in_use == n and s.csz == 32 and s.nch_used == 513 and s.nh - 512 * s.csz == 17
    for name, nh in (("tail_28_long_last_run", 35), ("tail_2_long_last_run", 19)):
        s = S[name]
        assert s.nh == nh and s.nh % 16 == 3 and s.n == nh - 1 + 30_000 and 14 in s.run_digits
        assert _column(name)[-30_000:] == _column(name)[-1:] * 30_000

    # the list after deep hits, once per register count
    assert [R.registers(n) for n in R.ORDER_SIZES] == list(range(1, 9))
    for n in R.ORDER_SIZES:
        s = S[f"order_{n}"]
        assert s.n_in_use == n and s.deepest_rank == n - 1 and min(R.ALPHABET[f"order_{n}"]) >= 0x80

    assert S[R.STALE[0]].n_in_use == 28 and S[R.STALE[1]].n_in_use == 5


@pytest.mark.parametrize("name", NAMES)
def test_emu_case(emu, oracle, name):
    _run_fresh(EMU_PATH, oracle, [name])


def test_emu_small_alphabet_behind_large(emu, oracle):
    _run_fresh(EMU_PATH, oracle, R.STALE)
    _run_fresh(EMU_PATH, oracle, R.STALE[::-1])


# ---------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(bzx, oracle, name):
    _run_fresh(LIB_PATH, oracle, [name])


@pytest.mark.gpu
def test_gpu_small_alphabet_behind_large(bzx, oracle):
    _run_fresh(LIB_PATH, oracle, R.STALE)
    _run_fresh(LIB_PATH, oracle, R.STALE[::-1])
