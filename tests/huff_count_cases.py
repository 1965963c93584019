"""Symbol streams for test_huffman_counts.py: the per-table symbol frequencies of the Huffman stage (bzx_huff.hip), which
counts the symbols 0 .. PACKED-1 of a group in packed register fields and every other symbol with an atomic of its own.
A case is (mtfv, alpha) as in huff_cases.py: uint16 symbols below alpha, the last one EOB (alpha - 1), once.  Streams
have at most about 30,000 symbols; every builder is deterministic.

a3_*          RUNA, RUNB and EOB only: EOB itself lies inside the packed range
solid_*       groups of 50 copies of one symbol: every symbol of the packed range and the first one above it
above_only    alpha = 258, nothing below the packed range but the EOB's group mates
boundary_pair alpha = 258, everything on the last packed symbol and the first unpacked one
last_1 / _49  a last group of EOB alone, and of 49 symbols
runa_*        n_mtf at the table-count thresholds, 90 % RUNA
few_groups    fewer groups than the kernel has lanes; sel_513 one group more than lanes
tie_packed    groups of packed symbols that cost the same under two tables in the first pass (first_pass_ties proves it)
"""
import random
from array import array

G = 50
PACKED = 9                      # HUF_PK of bzx_huff.hip: symbols 0 .. 8 are counted in register fields


def _finish(body, alpha):
    out = array("H", body)
    out.append(alpha - 1)
    return out, alpha


def two_runs(n_mtf, p_runa, seed):
    rnd = random.Random(seed)
    return _finish([0 if rnd.random() < p_runa else 1 for _ in range(n_mtf - 1)], 3)


def solid(symbols, alpha, per_symbol, seed):
    """per_symbol groups of 50 copies of each of `symbols`, the groups shuffled; EOB is a group of its own."""
    rnd = random.Random(seed)
    groups = [[s] * G for s in symbols for _ in range(per_symbol)]
    rnd.shuffle(groups)
    return _finish([s for g in groups for s in g], alpha)


def drawn(n_mtf, alpha, symbols, weights, seed):
    rnd = random.Random(seed)
    return _finish(rnd.choices(symbols, weights, k=n_mtf - 1), alpha)


def mostly_runa(n_mtf, alpha, seed):
    """90 % RUNA, the rest spread over the other symbols with geometric weights."""
    rest = list(range(1, alpha - 1))
    w = [0.9] + [0.1 * 0.5 ** (i + 1) for i in range(len(rest))]
    return drawn(n_mtf, alpha, [0] + rest, w, seed)


def tie_packed(n_groups_of_stream, seed):
    """Six symbols of equal frequency (alpha 7, all packed), at least 2,400 of them: six tables whose initial partitions
    hold one symbol each.  Every group is 25 copies of one symbol and 25 of another, shuffled: in the first pass it costs
    25 * 15 bits under either symbol's table and 50 * 15 under the others."""
    rnd = random.Random(seed)
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    groups = []
    for i in range(n_groups_of_stream):
        a, b = pairs[i % len(pairs)]
        g = [a] * (G // 2) + [b] * (G // 2)
        rnd.shuffle(g)
        groups.append(g)
    rnd.shuffle(groups)
    return _finish([s for g in groups for s in g], 7)


def first_pass_ties(mtfv, alpha):
    """Groups whose smallest first-pass cost is reached under two or more tables: libbz2's initial partition
    (hbAssignCodes' caller in compress.c sendMTFValues), lengths 0 inside a table's partition and 15 outside."""
    n = len(mtfv)
    n_tab = 2 if n < 200 else 3 if n < 600 else 4 if n < 1200 else 5 if n < 2400 else 6
    freq = [0] * alpha
    for s in mtfv:
        freq[s] += 1
    part, n_part, rem, gs = [None] * n_tab, n_tab, n, 0
    while n_part > 0:
        t_freq, ge, a_freq = rem // n_part, gs - 1, 0
        while a_freq < t_freq and ge < alpha - 1:
            ge += 1
            a_freq += freq[ge]
        if ge > gs and n_part != n_tab and n_part != 1 and (n_tab - n_part) % 2 == 1:
            a_freq -= freq[ge]
            ge -= 1
        part[n_part - 1] = (gs, ge)
        n_part -= 1
        gs = ge + 1
        rem -= a_freq
    ties = 0
    for g in range(0, n, G):
        cost = [sum(0 if lo <= s <= hi else 15 for s in mtfv[g:g + G]) for lo, hi in part]
        ties += cost.count(min(cost)) > 1
    return ties


def _cases():
    c = {}
    c["a3_even"] = lambda: two_runs(3001, 0.5, 1)
    c["a3_skewed"] = lambda: two_runs(2951, 0.97, 2)
    c["a3_eob_alone"] = lambda: two_runs(2501, 0.6, 3)                       # 50 groups of runs, then EOB alone
    c["solid_a11"] = lambda: solid(range(PACKED + 1), PACKED + 2, 6, 4)     # symbols 0 .. 9, EOB 10
    c["solid_a258"] = lambda: solid(list(range(PACKED + 1)) + [100, 256], 258, 5, 5)
    c["solid_last_packed"] = lambda: solid([PACKED - 1], 258, 60, 6)
    c["solid_first_unpacked"] = lambda: solid([PACKED], 258, 60, 7)
    c["above_only"] = lambda: drawn(20000, 258, list(range(PACKED, 257)), [0.97 ** i for i in range(257 - PACKED)], 8)
    c["boundary_pair"] = lambda: drawn(20000, 258, [PACKED - 1, PACKED], [0.6, 0.4], 9)
    c["last_1"] = lambda: mostly_runa(100 * G + 1, 40, 10)
    c["last_49"] = lambda: mostly_runa(100 * G + 49, 40, 11)
    for n in (199, 200, 599, 2399, 2400):
        c[f"runa_{n}"] = lambda n=n: mostly_runa(n, 30, 20 + n)
    c["few_groups"] = lambda: mostly_runa(37 * G + 13, 258, 12)
    c["sel_513"] = lambda: mostly_runa(512 * G + 20, 258, 13)
    c["sel_600_text_like"] = lambda: drawn(600 * G, 70, list(range(69)), [0.75 ** i for i in range(69)], 14)
    c["tie_packed"] = lambda: tie_packed(120, 15)
    return c


CASES = _cases()
