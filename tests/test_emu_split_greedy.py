"""CPU tests (-m "not gpu") of the split kernel's greedy bucket packing through the fiber emulator: the families of
test_split_greedy.py at 3,000 bytes (one segment, one or two buckets: the flag and id bookkeeping), and a few blocks of
70,000 to 100,000 bytes, which the emulator sorts in two to six seconds each: two and three segments, segments that
start at the same bin, the deeper split.  The rule is deterministic, so the emulator makes the buckets the device makes;
their number is compared with the numpy restatement."""
import bz2
import os
import subprocess

import pytest

import bsort_cases
import split_greedy_cases as cases
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


def check(emu, oracle, blk):
    L, orig, _ = emu.stage_bwt(blk)
    assert (L, orig) == oracle.bwt(blk), len(blk)
    assert emu.compress_buffer(blk, 9) == bz2.compress(blk, 9)
    st = emu.stats()
    assert st.n_unsorted == 0 and st.n_redo == 0
    assert st.n_buckets == cases.expected_items(blk)


def test_emu_fill(emu, oracle):
    check(emu, oracle, cases.fill_block(3000))


def test_emu_text(emu, oracle):
    check(emu, oracle, oracle.synthtext(3000))


def test_emu_exact_fits(emu, oracle):
    """2-bit symbols: 3,000 rotations in bins of a few ranks, a first bucket that ends within a rank or two of 2,048."""
    check(emu, oracle, cases.exact_fit_blocks(3000, 1)[0])


def test_emu_word(emu, oracle):
    check(emu, oracle, cases.with_word(oracle.synthtext(3000), 300))


def test_emu_heavy_bin(emu, oracle):
    check(emu, oracle, cases.heavy_bin_block(3000))


@pytest.mark.parametrize("k", [256, 2])
def test_emu_sparse_and_dense_bins(emu, oracle, k):
    check(emu, oracle, bsort_cases.alphabet_block(3000, k))


def test_emu_two_segments(emu, oracle):
    """70,000 bytes of text: two segments, 36 buckets."""
    check(emu, oracle, oracle.synthtext(70_000))


def test_emu_oversized_bin_among_small(emu, oracle):
    """A bin of 3,000 among the small bins of 70,000 bytes of text: the rule on the 4,096 bins of the deeper split."""
    blk = cases.with_word(oracle.synthtext(70_000), 3000)
    assert 3000 <= cases.max_bin(blk) < 3100
    check(emu, oracle, blk)


def test_emu_bin_larger_than_a_segment(emu, oracle):
    """40,000 of 100,000 rotations in one bin, three segments, two of which start at the same bin."""
    blk = cases.heavy_bin_block()
    assert cases.max_bin(blk) == 40_000
    check(emu, oracle, blk)
