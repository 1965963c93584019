"""Last columns for the tests of the MTF and zero-run stage (test_mtf_edges.py, on the device and through the
emulator): columns no BWT of ordinary input produces, each built to select one of the data-dependent paths of
bzx_mtf.hip.  A case is a zero-argument builder of the column L (bytes, 1..900,000 of them); every builder is
deterministic (random.Random(seed) only).  CASES maps name -> builder, GROUPS maps a group to its names:

tiny     n = 1, 2, 15, 16, 17; one run of 900,000 bytes; a first head of rank 0 alone and with a run; one not of rank 0
runs     run lengths 2^k - 2 .. 2^k + 1 (k = 1..16) over three symbols, the last run up to the block's last byte; runs
         whose zero-run numbers take 17 and 18 digits
tile1    run boundaries at the edges of pass 1's 16,384-byte tiles; n around a half tile, a tile and a tile + a lane
depth    cyclic columns in which every head has rank k - 1, k on both sides of every ranking variant, stride and NW
         boundary; five of them at 900,000 heads
chunks   head counts around 64 and 65 chunks (the second wave of the start lists), around the first chunk size of 32
         and around the last chunk of nch, at 2 and at 256 symbols
start    symbols that first appear late (the never-seen tail of the start lists), waves of chunks that bring nothing new,
         Zipf and uniform columns
staging  the most symbols a tile of pass 6 parks in LDS
odd      tiles of pass 6 that all emit an odd number of symbols: one waits in stg[0] at every tile start, and at EOB
full     900,000 uniform bytes, 900,000 Zipf bytes

mtf_reference() and mtf_inverse() are a plain Python model of the stage, written from the format; shape() mirrors the
kernel's arithmetic (chunking, variants, tiles) so that the test can prove which paths the cases reach."""
import random
from array import array
from collections import Counter
from typing import NamedTuple

# The constants of bzip2-rust_amd/csrc/bzx_mtf.hip (MTF_NT, MTF_E, MTF_LIST_BYTES, MTF_GROUP, and HE of its pass 6).
MTF_NT = 1024                   # lanes: chunks at most, heads per tile of pass 6 = MTF_NT * HE
MTF_E = 16                      # bytes per lane and tile of pass 1
HE = 8                          # heads per lane and tile of pass 6
MTF_LIST_BYTES = 72 * 1024      # half of the list pool
MTF_GROUP = 64                  # chunks of one wave
MAX_BLOCK = 900_000

TILE1 = MTF_NT * MTF_E          # 16,384 bytes
TILE6 = MTF_NT * HE             # 8,192 heads
RUNA, RUNB = 0, 1


# ---------------------------------------------------------------- the reference

def mtf_reference(L):
    """The stage from the format: (symbols as array('H'), freq[258], in_use[256])."""
    used = sorted(set(L))
    niu = len(used)
    dense = bytearray(256)
    in_use = bytearray(256)
    for i, b in enumerate(used):
        dense[b] = i
        in_use[b] = 1
    order = list(range(niu))
    out = array("H")
    run = 0

    def flush(run):
        # bijective base 2: run = sum of d_i * 2^i with digits d_i of 1 (RUNA) and 2 (RUNB), lowest first
        while run:
            if run & 1:
                out.append(RUNA)
                run = (run - 1) >> 1
            else:
                out.append(RUNB)
                run = (run - 2) >> 1

    for s in L.translate(bytes(dense)):
        r = order.index(s)
        if r == 0:
            run += 1
            continue
        flush(run)
        run = 0
        out.append(r + 1)
        order.insert(0, order.pop(r))
    flush(run)
    out.append(niu + 1)
    freq = [0] * 258
    for s in set(out):
        freq[s] = out.count(s)
    return out, freq, bytes(in_use)


def mtf_inverse(symbols, in_use):
    """The column a symbol stream stands for."""
    order = [b for b in range(256) if in_use[b]]
    eob = len(order) + 1
    out = bytearray()
    run, weight = 0, 1
    for s in symbols:
        if s <= RUNB:
            run += (s + 1) * weight
            weight <<= 1
            continue
        if run:
            out += bytes([order[0]]) * run
            run, weight = 0, 1
        if s == eob:
            return bytes(out)
        order.insert(0, order.pop(s - 1))
        out.append(order[0])
    raise ValueError("no EOB")


# ---------------------------------------------------------------- the kernel's shape arithmetic

def list_stride(niu):
    return (((niu + 7) // 8) | 1) * 8


def chunks_available(niu):
    pool = 2 * MTF_LIST_BYTES if niu > 64 else MTF_LIST_BYTES
    return min(MTF_NT, pool // list_stride(niu))


def chunking(niu, nh):
    """(stride, nch, csz, nch_used) of nh heads over niu symbols."""
    nch = chunks_available(niu)
    csz = (-(-nh // nch) + 15) & ~15
    return list_stride(niu), nch, csz, -(-nh // csz)


class Shape(NamedTuple):
    n: int
    n_in_use: int
    nh: int
    stride: int
    nch: int
    csz: int
    nch_used: int
    variant: str                # regs1..regs4: the list in 1..4 register words; lds: the four-word walk
    nw: int
    rec_in_lds: bool            # the recency lists: LDS up to 64 bytes in use, global memory above
    tiles1: int
    tiles6: int
    tile_counts: tuple          # symbols every tile of pass 6 emits
    max_staged: int             # the most a tile holds in LDS: the pending symbol and its own
    odd_tile_start: bool        # some tile after the first starts with an odd count so far
    odd_before_eob: bool
    deepest_rank: int
    spread_ranks: int           # ranks from 1 on that at least nh / (4 * n_in_use) heads take each
    first_rank0: bool
    run_digits: frozenset       # digit counts of the zero runs
    late_symbols: int           # symbols whose first head lies behind the first wave's chunks
    skipped_groups: int         # the most group lists a wave passes over in step B because they bring nothing new


def shape(L, symbols=None):
    n = len(L)
    used = sorted(set(L))
    niu = len(used)
    heads = [0] + [i + 1 for i, (a, b) in enumerate(zip(L, L[1:])) if a != b]
    nh = len(heads)
    stride, nch, csz, nch_used = chunking(niu, nh)
    variant = "lds" if niu > 32 else "regs%d" % ((niu + 7) // 8)
    nw = 1 if niu <= 64 else 2 if niu <= 128 else 4
    first_rank0 = L[0] == used[0]

    # pass 6: head k emits rank + 1 unless its rank is 0 (the first head alone can be), then the digits of the zeros
    # behind it: run - 1 of them, and the head itself if its rank is 0
    heads.append(n)
    counts, digits = [], set()
    for t0 in range(0, nh, TILE6):
        t1 = min(nh, t0 + TILE6)
        cnt = 0
        for k in range(t0, t1):
            z = heads[k + 1] - heads[k] - 1
            if k == 0 and first_rank0:
                z += 1
            else:
                cnt += 1
            if z:
                d = (z + 1).bit_length() - 1
                cnt += d
                digits.add(d)
        counts.append(cnt)
    carry, max_staged, odd_start = 0, 0, False
    for t, cnt in enumerate(counts):
        odd_start = odd_start or (t > 0 and carry & 1 == 1)
        max_staged = max(max_staged, (carry & 1) + cnt)
        carry += cnt

    if symbols is None:
        symbols = mtf_reference(L)[0]
    assert len(symbols) == carry + 1
    ranks = set(symbols[:-1])
    deepest = max(ranks) - 1 if ranks and max(ranks) > RUNB else 0
    hist = Counter(symbols[:-1])
    spread = sum(1 for s in ranks if s > RUNB and hist[s] * 4 * niu >= nh)

    # the start lists: the symbol set of every wave's 64 chunks, and step B's walk back over them
    dense = bytearray(256)
    for i, b in enumerate(used):
        dense[b] = i
    hs = bytes(dense[L[p]] for p in heads[:nh])
    masks = []
    for g0 in range(0, nh, csz * MTF_GROUP):
        m = 0
        for s in set(hs[g0:g0 + csz * MTF_GROUP]):
            m |= 1 << s
        masks.append(m)
    full = (1 << niu) - 1
    skipped = 0
    for w in range(1, len(masks)):
        seen, sk = 0, 0
        for g in range(w - 1, -1, -1):
            if seen == full:
                break
            if masks[g] & ~seen:
                seen |= masks[g]
            else:
                sk += 1
        skipped = max(skipped, sk)
    late = niu - bin(masks[0]).count("1")

    return Shape(n=n, n_in_use=niu, nh=nh, stride=stride, nch=nch, csz=csz, nch_used=nch_used, variant=variant, nw=nw,
                 rec_in_lds=niu <= 64, tiles1=-(-n // TILE1), tiles6=len(counts), tile_counts=tuple(counts),
                 max_staged=max_staged, odd_tile_start=odd_start, odd_before_eob=carry & 1 == 1, deepest_rank=deepest,
                 spread_ranks=spread, first_rank0=first_rank0, run_digits=frozenset(digits), late_symbols=late,
                 skipped_groups=skipped)


# ---------------------------------------------------------------- builders

def runs(lengths, symbols):
    """Runs of the given lengths, run i of symbols[i % len(symbols)] (neighbours in that cycle differ)."""
    return b"".join(bytes([symbols[i % len(symbols)]]) * l for i, l in enumerate(lengths))


def rnd(n, k, seed, base=0):
    """n bytes uniform over k values from base on."""
    r = random.Random(seed)
    return bytes(r.choices(range(base, base + k), k=n))


def zipf(n, k, seed, exponent=1.5):
    r = random.Random(seed)
    return bytes(r.choices(range(k), weights=[(i + 1) ** -exponent for i in range(k)], k=n))


def cyclic(k, n):
    return bytes(i % k for i in range(n))


def all_heads(nh, k, seed):
    """nh bytes over all k values in which no byte equals its neighbour: nh heads."""
    r = random.Random(seed)
    first = list(range(k))
    r.shuffle(first)
    out = bytearray(first[:nh]) + bytearray(r.choices(range(k), k=max(0, nh - k)))
    for i in range(k, nh):
        if out[i] == out[i - 1]:
            out[i] = (out[i] + 1) % k
    assert len(set(out)) == min(k, nh)
    return bytes(out)


def run_boundary(p, n, seed):
    """Three random symbols, with a 100-byte run that ends at position p - 1 and another that starts at p."""
    out = bytearray(rnd(n, 3, seed, base=40))
    out[p - 100:p] = bytes([77]) * 100
    out[p:p + 100] = bytes([78]) * 100
    return bytes(out)


def fill(prefix, symbol):
    """prefix, then one run of `symbol` up to the last byte of the largest block."""
    assert prefix[-1] != symbol
    return prefix + bytes([symbol]) * (MAX_BLOCK - len(prefix))


CASES = {}
GROUPS = {}


def _add(group, name, builder):
    assert name not in CASES
    CASES[name] = builder
    GROUPS.setdefault(group, []).append(name)


# tiny
_add("tiny", "n1", lambda: b"\x07")
_add("tiny", "n2", lambda: b"\x07\x03")
for _n in (15, 16, 17):
    _add("tiny", f"n{_n}", lambda n=_n: rnd(n, 3, 100 + n, base=9))
_add("tiny", "one_run_900000", lambda: bytes([200]) * MAX_BLOCK)
_add("tiny", "first_rank0_alone", lambda: bytes([3, 9, 5, 9, 3, 5, 5, 9, 9, 9, 3]))
_add("tiny", "first_rank0_run", lambda: bytes([3] * 6 + [9, 5, 9, 3, 3, 5, 9]))
_add("tiny", "first_not_rank0", lambda: bytes([9, 3, 5, 9, 3, 5, 5, 9, 9, 9, 3]))

# runs
_POW2 = [l for k in range(1, 17) for l in (2 ** k - 2, 2 ** k - 1, 2 ** k, 2 ** k + 1) if l]
_add("runs", "runs_pow2_k12", lambda: runs([l for l in _POW2 if l <= 2 ** 12 + 1], (5, 1, 250)))
_add("runs", "runs_pow2_fill", lambda: fill(runs(_POW2, (5, 1, 250)), (5, 1, 250)[len(_POW2) % 3]))
_add("runs", "run_digits_17_18", lambda: fill(runs([2 ** 17, 2 ** 18], (8, 2)), 5))

# tile1
for _p in (TILE1 - 1, TILE1, TILE1 + 1, 2 * TILE1 - 1, 2 * TILE1, 2 * TILE1 + 1):
    _add("tile1", f"run_at_{_p}", lambda p=_p: run_boundary(p, 50_000, p))
for _n in (8191, 8192, 8193, TILE1 - 1, TILE1, TILE1 + 1, TILE1 + 15, TILE1 + 16, TILE1 + 17):
    _add("tile1", f"alt_n{_n}", lambda n=_n: runs([1] * n, (6, 4)))
    _add("tile1", f"rnd3_n{_n}", lambda n=_n: rnd(n, 3, n, base=30))

# depth
CYCLIC = (2, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 64, 65, 72, 73, 80, 128, 129, 255, 256)
CYCLIC_FULL = (2, 33, 65, 129, 256)
for _k in CYCLIC:
    _add("depth", f"cyclic_{_k}", lambda k=_k: cyclic(k, 40_000 + k))
for _k in CYCLIC_FULL:
    _add("depth", f"cyclic_{_k}_full", lambda k=_k: cyclic(k, MAX_BLOCK))

# chunks: csz is 16 up to 16 * nch heads; 64 chunks are one wave
_NCH2, _NCH256 = chunks_available(2), chunks_available(256)
CHUNK_HEADS_2 = (1023, 1024, 1025, 1040, 1041, 16 * (_NCH2 - 1) + 1, 16 * _NCH2, 16 * _NCH2 + 1)
CHUNK_HEADS_256 = (1023, 1024, 1025, 1040, 1041, 16 * (_NCH256 - 1) + 1, 16 * _NCH256, 16 * _NCH256 + 1)
for _nh in CHUNK_HEADS_2:
    _add("chunks", f"alt_nh{_nh}", lambda nh=_nh: runs([1] * nh, (4, 6)))
for _nh in CHUNK_HEADS_256:
    _add("chunks", f"sym256_nh{_nh}", lambda nh=_nh: all_heads(nh, 256, nh))

# start
_add("start", "tail_400k_256", lambda: bytes(random.Random(11).choices((100, 200), k=400_000))
     + bytes(range(255, -1, -1)))
_add("start", "tail_60k_3", lambda: bytes(random.Random(12).choices((100, 200), k=60_000)) + bytes([150, 7, 250]))
_add("start", "stretch_200", lambda: rnd(50_000, 200, 13) + bytes(random.Random(14).choices((17, 170), k=100_000))
     + rnd(50_000, 200, 15))
_add("start", "zipf200_300k", lambda: zipf(300_000, 200, 16))
_add("start", "rnd_70001", lambda: random.Random(17).randbytes(70_001))

# staging: 8,192 heads of runs of 128 and 64 emit 5870 * 8 + 2322 * 7 = 63,214 symbols (the first head is not of rank 0)
_add("staging", "stage_bound", lambda: runs([128] * 5870 + [64] * 2322 + [1] * 32, (9, 4)))
# one single-byte run in front and the first tile emits an odd count, 1 + 5870 * 8 + 2320 * 7 + 6 = 63,207: a symbol
# is pending when the second tile starts (the block stays at 900,000 bytes)
_add("staging", "stage_bound_pending", lambda: runs([1] + [128] * 5870 + [64] * 2320 + [32] + [1] * 127, (9, 4)))

# odd: alternating symbols, one run of 2 in every tile of 8,192 heads
_add("odd", "odd_2tiles_odd_total", lambda: runs([2] + [1] * (TILE6 + 7), (9, 4)))
_add("odd", "odd_2tiles_even_total", lambda: runs([2] + [1] * (TILE6 - 1) + [1] * 3, (9, 4)))
_add("odd", "odd_3tiles", lambda: runs(([2] + [1] * (TILE6 - 1)) * 2 + [2] + [1] * 19, (9, 4)))
_add("odd", "odd_4tiles_even_total", lambda: runs(([2] + [1] * (TILE6 - 1)) * 3 + [2] + [1] * 19, (9, 4)))
_add("odd", "odd_stays_pending", lambda: runs([2] + [1] * (2 * TILE6 + 15), (9, 4)))

# full
_add("full", "rnd256_full", lambda: random.Random(18).randbytes(MAX_BLOCK))
_add("full", "zipf200_full", lambda: zipf(MAX_BLOCK, 200, 19))

BIG = "rnd256_full"                                      # the block that dirties a context
AFTER_BIG = GROUPS["tiny"] + ["tail_60k_3"]             # what has to come out clean behind it
