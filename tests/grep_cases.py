"""The model and the inputs of the grep tests (tests/test_grep.py, tests/test_cli_grep.py).

hits come from find_cases.hits (bytes.find in a loop).  line(p) = the number of delimiters in front of p: the cumulative
count of D == delim, looked up at each hit.  Grep comes from bytes.split: the records of D are D.split(delim) with the
delimiter put back behind all but the last, and a record matches when the pattern is in it."""
import bz2

import numpy as np

import find_cases as FC
import records_cases as RC


def lines_of(data, hit_list, delim):
    """[line(p) for p in hit_list]"""
    d = np.frombuffer(bytes(data), dtype=np.uint8)
    before = np.concatenate(([0], np.cumsum(d == delim, dtype=np.int64)))      # before[p] = delimiters in D[0, p)
    return [int(before[p]) for p in hit_list]


def seg_model(buf, segs, pat, delim):
    """bzx_stage_find_lines -> ([hit count], [delimiter count], [hits in segment order, relative to their segment],
    [the delimiters of the hit's own segment in front of it])"""
    counts, dcounts, allhits, alllines = [], [], [], []
    for off, ln in segs:
        seg = bytes(buf[off:off + ln])
        h = FC.hits(seg, pat)
        counts.append(len(h))
        dcounts.append(seg.count(bytes([delim])))
        allhits += h
        alllines += lines_of(seg, h, delim)
    return counts, dcounts, allhits, alllines


def records(data, delim):
    """The records of D with their terminating delimiters; the unterminated last one has none (and may be empty)."""
    parts = bytes(data).split(bytes([delim]))
    return [p + bytes([delim]) for p in parts[:-1]] + [parts[-1]]


def grep(data, pat, delim, listed=None):
    """-> ([record numbers], [record bytes]) of the records that hold a hit; listed: only the records of these hits."""
    recs = records(data, delim)
    if listed is None:
        nums = [i for i, r in enumerate(recs) if pat in r]
    else:
        nums = sorted(set(lines_of(data, listed, delim)))
    assert all(pat in recs[i] for i in nums)
    return nums, [recs[i] for i in nums]


def dense(n, seed, alphabet):
    """n seeded bytes over a small alphabet: hits and delimiters on every kind of border without planting."""
    a = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    return a[np.random.default_rng(seed).integers(0, len(a), n)].tobytes()


def planted_text(m, period=None, seed=21):
    """350,000 letters (seeded, or of period `period`), four level-1 blocks of 99,981, with newlines and a pattern of m
    letters around the cuts c = 99,981 k:
      k = 1  '\\n' is the last byte of block 0; the pattern starts on block 1's first byte
      k = 2  '\\n' is the first byte of block 2; a pattern ends on c - 1, another starts on c + 1
      k = 3  the pattern straddles the cut by half; a '\\n' directly in front of it (inside the m bytes before the cut)
             and one directly behind it (inside the m bytes behind the cut)
    and, far from every cut, a pattern with a newline on either side."""
    B = RC.BLOCK1
    pat = bytes(RC.letters(m, 100 + m))
    base = bytes(RC.letters(period or 350_000, seed))
    d = bytearray((base * (350_000 // len(base) + 1))[:350_000])
    c = B
    d[c - 1] = 10
    d[c:c + m] = pat
    c = 2 * B
    d[c - m:c] = pat
    d[c] = 10
    d[c + 1:c + 1 + m] = pat
    c = 3 * B
    s = c - m // 2
    d[s:s + m] = pat
    d[s - 1] = 10
    d[s + m] = 10
    d[5000] = 10
    d[5001:5001 + m] = pat
    d[5001 + m] = 10
    return bytes(d), pat


def straddle_text(period=997, seed=22):
    """The same 350,000 letters with a 17-byte pattern that CONTAINS '\\n' (8 letters, '\\n', 8 letters) planted across the
    cuts.  Where every block is a pass, the hit at c - 12 is found on the host in the carried 16 bytes [c - 16, c): the
    carry holds a delimiter in front of the hit's start (c - 15) and one behind it (the pattern's own, c - 4).  At the
    second cut the pattern's newline is the first byte behind the cut, at the third the last byte before it."""
    B = RC.BLOCK1
    pat = bytes(RC.letters(8, 31)) + b"\n" + bytes(RC.letters(8, 32))
    base = bytes(RC.letters(period or 350_000, seed))
    d = bytearray((base * (350_000 // len(base) + 1))[:350_000])
    d[B - 15] = 10
    d[B - 12:B + 5] = pat
    d[2 * B - 8:2 * B + 9] = pat
    d[3 * B - 9:3 * B + 8] = pat
    d[3 * B - 14] = 10
    return bytes(d), pat


def small_text():
    """An empty line that matches nothing, a line with three hits, a match in line 0 and one in the unterminated last."""
    return b"needle first\n\nno match here\nneedle, needle and needle\nplain\nlast needle without an end", b"needle"


def compress_streams(pieces):
    return b"".join(bz2.compress(p, 1) for p in pieces)
