"""Symbol streams for the seams of the emit stage (test_emit_tiles.py, through the emulator and on the device).

The emit kernel (bzx_emit.hip) cuts a block's payload into tiles of T 50-symbol groups, hands I consecutive tiles of a
block to a workgroup as one work item, packs a tile's bits in an LDS staging area of S bits and copies its words out.
T, I and S are the build's own (bzx_emit_geometry): nothing here carries a copy.  A case is (mtfv, alpha) as in
huff_cases.py.

seam<k>_last<l>   selector counts at the tile and item seams -- 1, 2, T-1, T, T+1, I*T-1, I*T, I*T+1, 2*I*T+1 and the
                  18,002 of the largest block -- each with a last group of 1, 49 and 50 symbols (the largest case is
                  cut to what a block can hold, seam_groups(): 18,001 groups ending in one symbol, 18,000 otherwise)
seed<k>           a few more streams of several tiles, which the word-seam coverage draws on
tile_spans()      where every tile of a block's payload starts and how many bits it has, from the oracle's tables and
                  selectors alone
"""
import ctypes as C

import huff_cases as H

G = H.G
LASTS = (1, 49, 50)
N_SEAMS = 10
MAX_SEL = 18002
SEEDED = ((3, 7, 258, 11), (2, 130, 90, 12), (5, 1, 258, 13), (1, 300, 40, 14))       # (tiles, groups more, alpha, seed)


def geometry(cdll):
    """(T groups per tile, I tiles per item, S staging bits) of a loaded libbzx build."""
    f = cdll.bzx_emit_geometry
    f.restype = None
    f.argtypes = [C.POINTER(C.c_uint32)] * 3
    t, i, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
    f(C.byref(t), C.byref(i), C.byref(s))
    return t.value, i.value, s.value


def seam_selectors(T, I):
    return (1, 2, T - 1, T, T + 1, I * T - 1, I * T, I * T + 1, 2 * I * T + 1, MAX_SEL)


def seam_groups(T, I, k, last):
    """Groups of seam case k: seam_selectors(T, I)[k], but no more than a block can have with a last group of `last`
    symbols.  A block holds 900,001 symbols at most: 18,001 groups, the last of one symbol, or 18,000 full ones (the
    18,002 of the selector arrays is libbz2's bound, which no block reaches)."""
    ns = seam_selectors(T, I)[k]
    while (ns - 1) * G + last > H.MAX_N_MTF:
        ns -= 1
    return ns


def seam_case(T, I, k, last):
    """Stream with seam_groups(T, I, k, last) groups, the last of `last` symbols (EOB included)."""
    ns = seam_groups(T, I, k, last)
    n = (ns - 1) * G + last
    return H.kinds(n, 258 if ns % 2 == 0 else 90, 7000 + n, 9 if ns >= MAX_SEL - 2 else 7)


def seeded_case(T, k):
    tiles, more, alpha, seed = SEEDED[k]
    return H.kinds((tiles * T + more) * G - seed, alpha, 9000 + seed)


def tile_spans(oracle, mtfv, alpha, T, sizes):
    """[(bit offset of the tile's first bit in the byte-aligned block image, bits of the tile)] for every tile.
    sizes: the section sizes the oracle's encoder reports (n_tables, n_selectors, map, selector, table, payload, total)."""
    gb = H.group_payloads(oracle, mtfv, alpha)
    assert len(gb) == sizes[1] and sum(gb) == sizes[5]
    pos = 105 + sizes[2] + 18 + sizes[3] + sizes[4]                     # header, map, nGroups/nSelectors, selectors, tables
    assert pos + sizes[5] == sizes[6]
    spans = []
    for g0 in range(0, len(gb), T):
        tot = sum(gb[g0:g0 + T])
        spans.append((pos, tot))
        pos += tot
    return spans
