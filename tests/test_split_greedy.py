"""Device tests of the split kernel's bucket packing (form_buckets in bzx_bsort.hip): bins are packed greedily into
buckets of at most 2,048 rotations, in up to 16 segments of the rank axis that one wave each walks.  How bins are
grouped cannot change the transform, so every case compares it with the oracle's and the stream with libbz2's, and no
block may fail the sortedness check or leave the bucket sorter; the number of work items is compared with a numpy
restatement of the rule (split_greedy_cases.expected_items)."""
import bz2

import pytest

import bsort_cases
import split_greedy_cases as cases

pytestmark = pytest.mark.gpu


def check(bzx, oracle, blk):
    """Transform, stream, no failed bucket, no block left to another sorter.  Returns the statistics of the stream."""
    L, orig, _ = bzx.stage_bwt(blk)
    assert (L, orig) == oracle.bwt(blk), len(blk)
    assert bzx.compress_buffer(blk, 9) == bz2.compress(blk, 9)
    st = bzx.stats()
    assert st.n_unsorted == 0 and st.n_redo == 0
    return st


def test_fill(bzx, oracle):
    """One full block of 32 letters without equal neighbours.  Inside a segment every bucket but the last is followed
    by a bin that did not fit, so it holds more than 2048 - m ranks (m: the largest bin); at most 16 segments.
    (m = 52, bound 467: the greedy rule makes 448 buckets, the window rule it replaced 503.)"""
    blk = cases.fill_block()
    n, m = len(blk), cases.max_bin(blk)
    st = check(bzx, oracle, blk)
    print(f"n {n} largest bin {m} buckets {st.n_buckets} bound {n // (2048 - m) + 17}")
    assert st.n_buckets <= n // (2048 - m) + 17
    assert st.n_buckets == cases.expected_items(blk)


@pytest.mark.parametrize("n", [30_000, 65_535, 65_536, 100_000, 524_287, 524_288, 899_981])
def test_segment_counts(bzx, oracle, n):
    """One segment; the step from one to two; three; the step from 15 to 16; a full block."""
    blk = oracle.synthtext(n)
    assert check(bzx, oracle, blk).n_buckets == cases.expected_items(blk)


def test_exact_fits(bzx, oracle):
    """Bins of one to three ranks: buckets that end at exactly 2,048 and at 2,047."""
    for blk in cases.exact_fit_blocks():
        assert check(bzx, oracle, blk).n_buckets == cases.expected_items(blk)


def test_oversized_bin_among_small(bzx, oracle):
    """One word 3,000 times: its bin goes through the deeper split (the rule on 4,096 bins), its neighbours are packed
    around it."""
    blk = cases.with_word(oracle.synthtext(200_000), 3000)
    assert 3000 <= cases.max_bin(blk) < 3100
    assert check(bzx, oracle, blk).n_buckets == cases.expected_items(blk)


def test_bin_larger_than_a_segment(bzx, oracle):
    """40,000 of 100,000 rotations in one bin, three segments: two of them start at the same bin and yield one bucket
    start."""
    blk = cases.heavy_bin_block()
    assert cases.max_bin(blk) == 40_000
    assert check(bzx, oracle, blk).n_buckets == cases.expected_items(blk)


@pytest.mark.parametrize("k", [256, 2])
def test_sparse_and_dense_bins(bzx, oracle, k):
    """256 symbols: most bins are empty and the search over the coarse prefixes iterates.  Two symbols: every bin is
    in use."""
    blk = bsort_cases.alphabet_block(70_000, k)
    assert check(bzx, oracle, blk).n_buckets == cases.expected_items(blk)
