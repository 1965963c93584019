"""CPU tests (-m "not gpu") of the paths of the bucket sort kernel through the fiber emulator: the families of
test_bsort_paths.py at sizes the emulator can afford (at most 3,000 bytes a block)."""
import bz2
import os
import subprocess

import pytest

import bsort_cases as cases
from bzx_ctypes import EMU_PATH, ROOT, BzxLib


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    lib = BzxLib(EMU_PATH)
    yield lib
    lib.close()


def check_bwt(emu, oracle, blk):
    L, orig, _ = emu.stage_bwt(blk)
    assert (L, orig) == oracle.bwt(blk), len(blk)


def test_emu_writeout_lengths(emu, oracle):
    """A slice of the device test's lengths 1..600 (the emulator takes 0.15 s a block): the shortest, those around a
    wave's and a workgroup's row of lanes, and eight in a row at the top -- every residue mod 8 twice over."""
    blocks = cases.writeout_lengths()
    for n in list(range(1, 13)) + [63, 64, 65, 255, 256, 257, 511, 512, 513] + list(range(593, 601)):
        check_bwt(emu, oracle, blocks[n - 1])


def test_emu_writeout_full_bucket(emu, oracle):
    check_bwt(emu, oracle, cases.letters(3000, b"acgt", 12))


@pytest.mark.parametrize("n", [257, 511, 513, 2049, 3000])
def test_emu_lsd_rows(emu, oracle, n):
    check_bwt(emu, oracle, oracle.synthtext(n))


def test_emu_lsd_digit_skipping(emu, oracle):
    check_bwt(emu, oracle, cases.long_runs(3000))


@pytest.mark.parametrize("k", [2, 17, 256])
def test_emu_lsd_alphabets(emu, oracle, k):
    check_bwt(emu, oracle, cases.alphabet_block(3000, k))


@pytest.mark.parametrize("base,length,copies", [(2900, 25, 3), (1200, 25, 70), (2900, 45, 2)])
def test_emu_short_list_rounds(emu, oracle, base, length, copies):
    """As on the device; the 70 copies leave groups of 70 ranks tied after round 0, a list above 64 for round 1."""
    check_bwt(emu, oracle, cases.with_phrase(oracle.synthtext(base), length, copies))


def test_emu_short_list_gives_up(emu, oracle):
    blk = cases.with_copy(oracle.synthtext(2600), 700, 300)
    check_bwt(emu, oracle, blk)
    assert emu.compress_buffer(blk, 9) == bz2.compress(blk, 9)
    st = emu.stats()
    assert st.n_open_buckets > 0 and st.n_unsorted == 0
