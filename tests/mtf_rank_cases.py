"""Last columns for the tests of the register rank loop of bzx_mtf.hip (test_mtf_rank_regs.py): alphabets of at most 32
byte values, whose MTF list a lane keeps in NR = ceil(n_in_use / 4) 32-bit registers of four entries.  A case is a
zero-argument builder of the column (bytes, at most about 40,000); CASES maps name -> builder, GROUPS a group to its
names, ALPHABET a name to the sorted byte values the column is built over.  Everything is deterministic.

A column is written as a sequence of MTF ranks over an alphabet: from_ranks() plays the move-to-front backwards (the
list starts out as the alphabet in ascending order; rank r names the entry at position r, which then moves to the
front), so a builder says which list entry every head hits.  A head of rank >= 1 differs from its predecessor, so every
rank >= 1 is one run head.

every    every n_in_use of SIZES over low bytes, bytes from 0xE0 on and scattered bytes: the heads take the ranks
         1 .. n_in_use - 1 in turn, again and again -- a hit in every byte of every register, padding next to live
         entries where n_in_use is no multiple of 4; the first head has rank 1
first0   the first byte is the smallest in use: the only head of rank 0
tails    head counts 1, 15, 16, 17, 31, 32, 33, 47, 49 over alphabets of 2 and of 28 values (a column of nh heads uses
         at most nh values: the small ones use what they can), 16,401 heads (chunks of 32, the last with 17), and a
         column whose short last group is followed by one run of 30,000 bytes
order    after a head of rank n_in_use - 1 the next heads take the ranks 1, 2, 3, ...: once per register count"""
import random

SIZES = (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 31, 32)
ORDER_SIZES = (4, 8, 12, 16, 20, 24, 28, 32)            # NR = 1 .. 8
TAIL_HEADS = (1, 15, 16, 17, 31, 32, 33, 47, 49)


def registers(n_in_use):
    """NR of the kernel's dispatch."""
    return (n_in_use + 3) // 4


def low(n):
    return list(range(1, n + 1))


def high(n):
    """The last n byte values of 0xE0 .. 0xFF."""
    return list(range(0x100 - n, 0x100))


def scattered(n):
    """n byte values from all over, both halves of the byte range among them."""
    r = random.Random(4000 + n)
    lo = n // 2
    return sorted(r.sample(range(0x80), lo) + r.sample(range(0x80, 0x100), n - lo))


def from_ranks(alphabet, ranks, run_of=lambda i: 1):
    """The column whose heads have the given ranks (the first may be 0, every other is >= 1); head i is a run of
    run_of(i) bytes."""
    order = list(alphabet)
    out = bytearray()
    for i, r in enumerate(ranks):
        assert r < len(order) and (r or i == 0)
        order.insert(0, order.pop(r))
        out += bytes([order[0]]) * run_of(i)
    return bytes(out)


def _runs(i):
    return 3 if i % 7 == 3 else 2 if i % 5 == 1 else 1


def every_rank(alphabet, heads=2400):
    n = len(alphabet)
    ranks = [1 + i % (n - 1) for i in range(heads + n)]
    return from_ranks(alphabet, ranks, _runs)


def deep_then_up(alphabet):
    n = len(alphabet)
    ranks = []
    for j in range(1, n - 1):
        ranks += [n - 1] + list(range(1, j + 1))
    return from_ranks(alphabet, ranks * 3, _runs)


def heads_over(alphabet, nh, last_run=1):
    """nh heads that bring in as many values of the alphabet as nh allows, deepest ranks first; the last head is a run
    of last_run bytes."""
    n = min(len(alphabet), nh)
    ranks = [0] + [n - 1] * (n - 1) if n > 1 else [0]
    ranks += [1 + (5 * i) % (n - 1) for i in range(nh - len(ranks))] if n > 1 else []
    assert len(ranks) == nh
    return from_ranks(alphabet[:n], ranks, lambda i: last_run if i == nh - 1 else 1)


CASES = {}
GROUPS = {}
ALPHABET = {}


def _add(group, name, alphabet, builder):
    assert name not in CASES
    CASES[name] = builder
    ALPHABET[name] = alphabet
    GROUPS.setdefault(group, []).append(name)


for _n in SIZES:
    for _kind, _mk in (("low", low), ("high", high), ("scat", scattered)):
        _add("every", f"every_{_kind}_{_n}", _mk(_n), lambda a=_mk(_n): every_rank(a))

for _n in (5, 28):
    _add("first0", f"first0_{_n}", high(_n), lambda a=high(_n): from_ranks(a, [0] + [1 + i % (len(a) - 1) for i in range(600)], _runs))

for _n in (2, 28):
    for _nh in TAIL_HEADS:
        _add("tails", f"tail_{_n}_nh{_nh}", scattered(_n)[:min(_n, _nh)], lambda a=scattered(_n), nh=_nh: heads_over(a, nh))
    _add("tails", f"tail_{_n}_nh16401", scattered(_n), lambda a=scattered(_n): heads_over(a, 16401))
_add("tails", "tail_28_long_last_run", scattered(28), lambda a=scattered(28): heads_over(a, 35, last_run=30_000))
_add("tails", "tail_2_long_last_run", scattered(2), lambda a=scattered(2): heads_over(a, 19, last_run=30_000))

for _n in ORDER_SIZES:
    _add("order", f"order_{_n}", high(_n), lambda a=high(_n): deep_then_up(a))

STALE = ("every_scat_28", "every_high_5")               # a 28-symbol column and a 5-symbol column, run back to back
