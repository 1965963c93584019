"""Device tests of the paths of the bucket sort kernel (bzx_bsort.hip): the last-column write-out in rotated slot order,
the two-barrier LSD passes of the initial sort, and the refinement rounds that one wave runs when the list of tied ranks
is short.  Every block's transform is compared with the oracle's; one stream per family with libbz2's."""
import bz2

import pytest

import bsort_cases as cases

pytestmark = pytest.mark.gpu


def check_bwt(bzx, oracle, blk):
    L, orig, _ = bzx.stage_bwt(blk)
    assert (L, orig) == oracle.bwt(blk), len(blk)


def check_stream(bzx, data):
    assert bzx.compress_buffer(data, 9) == bz2.compress(data, 9)
    assert bzx.stats().n_unsorted == 0


def test_writeout_every_length(bzx, oracle):
    """Lengths 1..600: the ragged tail of a bucket at every residue mod 8, and rotation 0 (orig_ptr) in each of the eight
    slots a lane visits."""
    blocks = cases.writeout_lengths()
    for blk in blocks:
        check_bwt(bzx, oracle, blk)
    check_stream(bzx, blocks[-1])


def test_writeout_full_buckets(bzx, oracle):
    """Four letters, 40,000 rotations: buckets that fill all 2,048 ranks, every lane of the write-out busy."""
    blk = cases.letters(40_000, b"acgt", 12)
    check_bwt(bzx, oracle, blk)
    check_stream(bzx, blk)


@pytest.mark.parametrize("n", [257, 511, 513, 2049, 60_000])
def test_lsd_rows(bzx, oracle, n):
    """Partial rows, one row, all rows of the initial sort's passes."""
    check_bwt(bzx, oracle, oracle.synthtext(n))


def test_lsd_digit_skipping(bzx, oracle):
    """Records that agree on whole key digits: those passes are skipped."""
    blk = cases.long_runs(20_000)
    check_bwt(bzx, oracle, blk)
    check_stream(bzx, blk)


@pytest.mark.parametrize("k", [2, 17, 256])
def test_lsd_alphabets(bzx, oracle, k):
    check_bwt(bzx, oracle, cases.alphabet_block(30_000, k))


def test_lsd_stream(bzx, oracle):
    check_stream(bzx, oracle.synthtext(60_000))


@pytest.mark.parametrize("length,copies", [(25, 3), (25, 150), (45, 2)])
def test_short_list_rounds(bzx, oracle, length, copies):
    """A 25-symbol phrase three times: resolved in round 1 on a list of a few ranks (one wave).  150 times: the list of
    round 1 is above 64 and the workgroup still runs it.  45 symbols twice: rounds 2-3 on the wave."""
    blk = cases.with_phrase(oracle.synthtext(20_000), length, copies)
    check_bwt(bzx, oracle, blk)
    if copies == 3:
        check_stream(bzx, blk)


def test_short_list_gives_up(bzx, oracle):
    """A 300-symbol stretch twice: its bucket gives up from the one-wave rounds and the rank rounds finish the block."""
    blk = cases.with_copy(oracle.synthtext(20_000), 5000, 300)
    check_bwt(bzx, oracle, blk)
    check_stream(bzx, blk)
    assert bzx.stats().n_open_buckets > 0
