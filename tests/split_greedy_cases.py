"""Blocks for the tests of the split kernel's greedy bucket packing (test_split_greedy.py on the device,
test_emu_split_greedy.py through the emulator), and a restatement of the packing rule in numpy: the number of work
items the split stage must hand to the sort kernel for a block.  Every builder is deterministic."""
import random

import numpy as np

BS_C = 2048          # rotations per bucket
BIN1, BIN2 = 15, 12  # key bits of the level-1 bins and of the deeper levels
NW = 16              # waves of the split kernel's workgroup: at most this many segments


def fill_block(n=899_981, seed=2024):
    """32 letters, no two equal neighbours (RLE1 is the identity): every 3-symbol prefix is rare, bins are small."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(1, 32, size=n, dtype=np.int64)          # 1..31: never the same letter again
    return ((int(rng.integers(0, 32)) + np.cumsum(steps)) % 32 + 64).astype(np.uint8).tobytes()


def exact_fit_blocks(n0=40_000, count=8, seed=12):
    """Four letters at eight consecutive lengths: 2-bit symbols, bins of one to three ranks, so buckets end at exactly
    BS_C and at BS_C - 1 somewhere in every block."""
    rnd = random.Random(seed)
    data = bytes(rnd.choice(b"acgt") for _ in range(n0 + count - 1))
    return [data[:n0 + i] for i in range(count)]


def with_word(text, copies, seed=3):
    """The word "qzj" `copies` times, each followed by three varying letters, written over the text at even distances
    (the text's own few occurrences come on top).  No run of four equal bytes arises."""
    rnd = random.Random(seed)
    out = bytearray(text)
    step = len(text) // copies
    assert step >= 8
    for i in range(copies):
        tail, prev = [], ord("j")
        for _ in range(3):
            c = rnd.choice([x for x in b"abcdefghijklmnopqrstuvwxyz" if x != prev])
            tail.append(c)
            prev = c
        at = i * step + 1
        out[at:at + 6] = b"qzj" + bytes(tail)
    return bytes(out)


def heavy_bin_block(n=100_000, seed=9):
    """Exactly 2 n / 5 of the n rotations start with "aba" (n a multiple of 5): units of "abab...a" (k letters a) and r
    other letters with sum(k) = sum(3 + 2 r); 32 symbols in all, so a bin is three symbols.  The units vary in k, r and
    their letters, so no stretch of 45 symbols occurs twice (asserted)."""
    assert n % 5 == 0
    rnd = random.Random(seed)
    others = bytes(range(ord("c"), ord("c") + 30))
    left = n // 5                  # a pair of units (r1, d), (r2, -d) is 5 (2 + r1 + r2) bytes long
    out = bytearray()
    while left:
        if left >= 12:
            r1, r2 = rnd.randint(1, 3), rnd.randint(1, 3)
        elif left > 8:
            r1, r2 = 1, left - 4 - 3
        else:
            assert left >= 4
            r1, r2 = (left - 2 + 1) // 2, (left - 2) // 2
        left -= 2 + r1 + r2
        d = rnd.choice((-1, 0, 1))
        for r, dd in ((r1, d), (r2, -d)):
            k = 3 + 2 * r + dd
            out += b"ab" * (k - 1) + b"a" + bytes(rnd.choice(others) for _ in range(r))
    blk = bytes(out)
    assert len(blk) == n and len(set(blk)) == 32
    two = blk + blk[:45]
    assert len({two[i:i + 45] for i in range(n)}) == n
    return blk


def rle1(blk):
    """bzip2's first run-length stage (runs of 4..255 equal bytes -> four bytes and a count)."""
    a = np.frombuffer(blk, dtype=np.uint8)
    if len(a) < 4 or not np.any((a[3:] == a[:-3]) & (a[2:-1] == a[:-3]) & (a[1:-2] == a[:-3])):
        return blk
    out = bytearray()
    i, n = 0, len(blk)
    while i < n:
        j = i
        while j < n and blk[j] == blk[i] and j - i < 255:
            j += 1
        run = j - i
        if run >= 4:
            out += blk[i:i + 4] + bytes([run - 4])
        else:
            out += blk[i:j]
        i = j
    return bytes(out)


def greedy_starts(counts):
    """First bins of the buckets the rule makes of these bin counts (ISSUE: segmented greedy packing)."""
    incl = np.cumsum(counts, dtype=np.int64)
    total, bins = int(incl[-1]), len(counts)
    nseg = min(max(total // (16 * BS_C), 1), NW)
    # segment k starts at the first bin whose EXCLUSIVE prefix is >= ceil(k total / nseg)
    seg = [0] + [int(np.searchsorted(incl, -(-k * total // nseg), "left")) + 1 for k in range(1, nseg)] + [bins]
    starts = set()
    for k in range(nseg):
        s, end = seg[k], min(seg[k + 1], bins)
        while s < end:
            starts.add(s)
            base = int(incl[s - 1]) if s else 0
            j = int(np.searchsorted(incl, base + BS_C + 1, "left"))      # first bin that no longer fits
            s = s + 1 if j <= s else j
    return sorted(starts)


def expected_items(blk):
    """Work items (buckets, oversized bins included) of the block: level 1 and every deeper split."""
    blk = rle1(blk)
    a = np.frombuffer(blk, dtype=np.uint8)
    n = len(a)
    syms = np.unique(a)
    bits = 1
    while (1 << bits) < len(syms):
        bits += 1
    ids = np.searchsorted(syms, a)
    bitstr = ((ids[:, None] >> np.arange(bits - 1, -1, -1)) & 1).astype(np.uint8).reshape(-1)
    nb = n * bits

    def keys(rots, depth, width):
        pos = (rots * bits + depth)[:, None] + np.arange(width)
        return (bitstr[pos % nb].astype(np.int64) << np.arange(width - 1, -1, -1)).sum(axis=1)

    items = 0
    work = [(np.arange(n, dtype=np.int64), 0, BIN1)]
    while work:
        rots, depth, width = work.pop()
        assert depth + width + 32 < nb and depth + width <= 511, "beyond what this restatement covers"
        k = keys(rots, depth, width)
        counts = np.bincount(k, minlength=1 << width)
        starts = greedy_starts(counts)
        items += len(starts)
        assert len(starts) <= 1024
        for b in np.nonzero(counts > BS_C)[0]:
            work.append((rots[k == b], depth + width, BIN2))
    return items


def max_bin(blk):
    """Largest count of any level-1 bin, for blocks of 32 symbols: of any 3-symbol prefix over all rotations."""
    a = np.frombuffer(blk, dtype=np.uint8).astype(np.int64)
    syms = np.unique(a)
    assert 16 < len(syms) <= 32
    ids = np.searchsorted(syms, a)
    k = (ids << 10) | (np.roll(ids, -1) << 5) | np.roll(ids, -2)
    return int(np.bincount(k, minlength=1 << 15).max())
