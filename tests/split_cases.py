"""Raw inputs for the tests of the first stage (test_split_edges.py, on the device and through the emulator): RLE1,
the block splitter and the block CRCs of bzx_rle1.hip / bzx_rle1.h, the segmented copy of them in bzx_batch.hip and
the chunked entry bzx_split_rle1_chunk.  Every input is built to put one of the stage's data-dependent paths on a
lane, tile, block, segment or 16-byte edge.  A case is a Case(build, level, emu, big); build() returns the input as
bytes and is deterministic.  CASES maps name -> Case, GROUPS maps a group to its names:

pieces   tiny inputs; runs of 1..6, 254..260, 509..512 and 768..770 bytes as the whole input, at its start, at its end
         and twice in a row; a 4-run that ends the input (count 0); a count of 251
edges    4-runs that end -3..+3 bytes around a lane edge, the edge of tiles 0/1 and of tiles 1/2; 3-runs across a tile
         edge; the two-byte write of a piece's 4th byte on a tile's last byte; a 251-byte look-ahead across a tile
         edge; a 255 cut on a tile edge (a tile kernel A flags and kernel B clears); runs over whole tiles; lengths
         around one and two tiles; ragged last lanes; a one-byte last tile
full     the RLE1 length of the input at nmax - 1, nmax, nmax + 1, 2 nmax; the block filled at a plain byte, at k = 0,
         1, 2, over the two-byte step of k = 3, inside a swallowed stretch, by a piece that a 255 cut ends, by a piece
         that ends the input, at the first byte of the next tile; a piece end across a tile edge; blocks of nmax + 4
         bytes at levels 1 and 9; the densest expansion
chain    the batched window path with J = 2, 3 and 64, with a drifting window, refused by one flagged tile; the single
         fast path refused by the end of the input; plain and non-plain last blocks; one flagged tile at either end;
         plain and non-plain blocks in turn
scans    tile counts around two segments of the scans (SCAN_SEG = 16 in the emulator build, 8192 shipped)
crc      single blocks of 1 .. 131,073 bytes; 17 plain level-1 blocks whose starts visit all residues mod 16

Which k the block-full position x can have: x is the smallest position with F(x) >= target, so the byte before it
emitted something (k <= 3) and x has k in {0 at a run start, 1, 2, 3, 4}.  A position with k = 254, or the first byte
behind a 255 cut, follows a byte that emits nothing and is never x; what a block CAN do there is end with a piece whose
last byte has k = 254, so that the next block starts behind the cut inside the same run (full_cut_*).

reference() is a whole-array numpy model of libbz2's rule, written from the rule and not from the kernels' tiling;
trace() mirrors the kernels' path decisions (and nothing of their arithmetic on bytes) so that the test can prove
which paths the cases reach."""
import re
import zlib
from typing import NamedTuple

import numpy as np

# The constants of bzip2-rust_amd/csrc/bzx_rle1.h and bzx_rle1.hip (test_constants_match_the_sources parses them).
RL_NT = 256
RL_BYTES = 32
RL_TILE = RL_NT * RL_BYTES          # 8192
BND_J = 64                          # blocks per batch of the window path
BND_W = 4 * BND_J + 16              # window bytes per predicted boundary
CRC_TILE = 1024 * 64                # 64 KiB
SCAN_SEG = 8192                     # shipped; SCAN_ITER entries per loop iteration of the scan kernel
SCAN_SEG_EMU = 16                   # -DSCAN_SEG of tests/emu/build_emu.sh
SCAN_ITER = 1024 * 8
MAX_BLOCK = 900_000

T = RL_TILE


def nmax(level):
    return 100000 * level - 19


N1 = nmax(1)


def max_blocks(n, level):
    """The splitter's bound on the block count (split_on_device)."""
    return (n + n // 4) // nmax(level) + 2


def parse_constants(header_text, source_text, emu_script_text):
    """The #define lines of the two sources and the -DSCAN_SEG flag of the emulator build -> dict of the mirrored names."""
    env = {}
    for text in (header_text, source_text):
        for m in re.finditer(r"^#define\s+(\w+)\s+([^/\n]+?)\s*(?://.*)?$", text, re.M):
            name, expr = m.group(1), m.group(2)
            if re.fullmatch(r"[\w\s()*+\-]+", expr):
                try:
                    env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
                except Exception:
                    pass
    flags = set(re.findall(r"-DSCAN_SEG=(\d+)", emu_script_text))
    assert len(flags) == 1, flags
    env["SCAN_SEG_EMU"] = int(flags.pop())
    return env


# ---------------------------------------------------------------- the reference

REV8 = bytes(int(f"{b:08b}"[::-1], 2) for b in range(256))


def crc_bzip2(d):
    """CRC-32/BZIP2 is the unreflected twin of zlib's CRC-32: reflect every byte going in and the word coming out."""
    c = zlib.crc32(bytes(d).translate(REV8))
    return int(f"{c:032b}"[::-1], 2)


def model(a):
    """Per position of the uint8 array a: run start flag, k = (p - run start) % 255, emitted bytes e; F[p] = bytes
    emitted before p (F has len(a) + 1 entries)."""
    n = len(a)
    idx = np.arange(n, dtype=np.int64)
    new = np.ones(n, dtype=bool)
    new[1:] = a[1:] != a[:-1]
    rs = np.maximum.accumulate(np.where(new, idx, 0))
    k = (idx - rs) % 255
    e = np.where(k < 3, 1, np.where(k == 3, 2, 0)).astype(np.int64)
    F = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(e, out=F[1:])
    return new, rs, k, e, F


def rule_bounds(k, F, n, level):
    """libbz2's split rule on the whole arrays: [(raw_lo, raw_hi, x)] with x the position that filled the block
    (None for a last block that never fills)."""
    ps = np.flatnonzero(k == 0)
    out, start, N = [], 0, nmax(level)
    while start < n:
        target = F[start] + N
        x = None
        if F[n] < target:
            q = n
        else:
            x = int(np.searchsorted(F, target, "left"))
            i = int(np.searchsorted(ps, x, "left"))
            q = int(ps[i]) if x < n and i < len(ps) else n
        out.append((start, q, x))
        start = q
    return out


def reference(data, level):
    """[(image, crc, raw_lo, raw_hi)] of every block of data."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(a)
    if n == 0:
        return []
    new, rs, k, e, F = model(a)
    ps = np.flatnonzero(k == 0)                  # piece starts; a piece ends where the next one starts
    pe = np.append(ps[1:], n)
    img = np.zeros(int(F[n]), dtype=np.uint8)
    em = np.flatnonzero(e)
    img[F[em]] = a[em]
    four = np.flatnonzero(e == 2)                # the 4th byte of a piece is followed by the count of the rest
    pi = np.searchsorted(ps, four, "right") - 1
    img[F[four] + 1] = (pe[pi] - ps[pi] - 4).astype(np.uint8)
    return [(img[F[lo]:F[hi]].tobytes(), crc_bzip2(data[lo:hi]), lo, hi) for lo, hi, _ in rule_bounds(k, F, n, level)]


def raw_lengths(data, level):
    """raw_hi - raw_lo of every block of data (the rule alone, no images)."""
    if not data:
        return []
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    new, rs, k, e, F = model(a)
    return [hi - lo for lo, hi, _ in rule_bounds(k, F, len(a), level)]


# ---------------------------------------------------------------- the trace

class Block(NamedTuple):
    lo: int
    hi: int
    path: str          # "batch", "single", "search", "last"
    J: int             # blocks of the batch (batch only)
    woff: int          # offset of the boundary's window (batch only)
    x: int             # the position that filled the block (-1: last)
    k_x: int           # k there (-1: x >= len or last)
    x_next_tile: bool  # search: x is the first byte of the tile behind the one that was scanned
    x_newrun: bool     # ... and starts a run
    x_ge_len: bool     # search: x >= len
    end_crossed: bool  # search: piece_end read across a tile edge
    plain: bool        # the flag the chain leaves: the block is read in place
    refused: str       # why a faster path was not taken: "", "np" (a flagged tile), "len:<d>" (x + 4 - d == len)
    n: int             # RLE1 length
    over: int = -1     # search, x < len: F(x) - target, 0 or 1 (1: the two-byte step of a 4th byte jumped the target)
    step: int = -1     # search, x < len: what the byte before x emitted, 1 or 2
    x_run2: bool = False   # search, x < len: x starts a run of two or more bytes


class Trace(NamedTuple):
    n: int
    ntiles: int
    flag_a: np.ndarray      # per tile: kernel A's provisional flag
    flag_b: np.ndarray      # per tile: the exact flag kernel B leaves
    carry: np.ndarray       # per tile: run start (+1) carried into it
    own_rs: np.ndarray      # per tile: it holds a run start of its own
    blocks: list
    batch_refused: int      # times the batched path was refused by a flagged tile
    ev_p: np.ndarray        # scatter events (4th bytes of pieces): position,
    ev_extra: np.ndarray    # look-ahead length,
    ev_cross: np.ndarray    # the look-ahead read across a tile edge,
    ev_block_end: np.ndarray   # the two-byte write ends a block
    scan: tuple             # (levels, loop iterations of a first-level workgroup, segments, last segment's length)
    crc: list               # per block (lo % 16, length, the bytewise partial piece is taken)


def scan_shape(ntiles, seg):
    if ntiles <= 2 * seg:
        return (1, max(1, -(-ntiles // SCAN_ITER)), 1, ntiles)
    nseg = -(-ntiles // seg)
    return (2, -(-seg // SCAN_ITER), nseg, ntiles - (nseg - 1) * seg)


def trace(data, level, scan_seg=SCAN_SEG):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(a)
    assert n
    N = nmax(level)
    new, rs, k, e, F = model(a)
    nt = -(-n // T)
    tiles = np.arange(nt)

    def per_tile(v):
        p = np.zeros(nt * T, dtype=bool)
        p[:n] = v
        return p.reshape(nt, T).any(axis=1)

    eq4 = np.zeros(n, dtype=bool)                # four equal bytes end here
    if n >= 4:
        eq4[3:] = (a[3:] == a[2:-1]) & (a[2:-1] == a[1:-2]) & (a[1:-2] == a[:-3])
    inner = (tiles > 0) & ((tiles + 1) * T <= n)
    flag_a = np.where(inner, per_tile(eq4), True)
    flag_b = per_tile(k >= 3)
    assert not (flag_b & ~flag_a).any()          # A's test is conservative
    carry = np.zeros(nt, dtype=np.int64)
    carry[1:] = rs[tiles[1:] * T - 1] + 1
    own_rs = per_tile(new)
    npc = np.concatenate(([0], np.cumsum(flag_b)))   # tile_np after its scan

    def k_before(x):                             # the fast paths' k: equal bytes right before x, at most 3
        kk = 0
        while kk < 3 and a[x - 1 - kk] == a[x]:
            kk += 1
        return kk

    def fast_end(x, kk):
        q = x
        if kk:
            q = x + 1
            while kk + (q - x) < 4 and q < x + 4 and a[q] == a[x]:
                q += 1
        return q

    blocks, start, f_start, nb, refusals = [], 0, 0, 0, 0
    mb = max_blocks(n, level)
    f_len = int(F[n])
    while start < n and nb < mb:
        J = BND_J
        room = (n - start - BND_W - 16) // N if n > start + BND_W + 16 else 0
        if room < J + 1:
            J = room - 1 if room > 1 else 0
        if nb + J > mb:
            J = mb - nb
        why = ""
        if J >= 2:
            last = start + (J + 1) * N + 4 * J + 8
            if npc[min(last // T + 2, nt)] != npc[start // T]:
                J, why = 0, "np"
                refusals += 1
        if J >= 2:
            start0 = start
            for j in range(J):
                x = start + N
                woff = start - (start0 + j * N)
                assert 0 <= woff and woff + 8 <= BND_W and x + 3 < n
                kk = k_before(x)
                q = fast_end(x, kk)
                blocks.append(Block(start, q, "batch", J, woff, x, kk, False, False, False, False, True, "", q - start))
                f_start += q - start
                start = q
                nb += 1
            continue
        nb += 1
        target = f_start + N
        if f_len < target:
            blocks.append(Block(start, n, "last", 0, 0, -1, -1, False, False, False, False,
                                bool(npc[nt] == npc[start // T]), why, f_len - f_start))
            start, f_start = n, f_len
            break
        x = start + N
        if x >= 4 and npc[min(x // T + 2, nt)] == npc[start // T]:
            if x + 4 < n:
                kk = k_before(x)
                q = fast_end(x, kk)
                blocks.append(Block(start, q, "single", 0, 0, x, kk, False, False, False, False, True, why, q - start))
                f_start += q - start
                start = q
                continue
            why = "len:%d" % (x + 4 - n)
        elif not why:
            why = "np"
        # the search: last tile whose F at its start is below the target, one scan of it
        tile = int(np.searchsorted(F[tiles * T], target, "left")) - 1
        lo_, hi_ = tile * T, min((tile + 1) * T, n)
        inside = np.flatnonzero(F[lo_:hi_] >= target)
        x = lo_ + int(inside[0]) if len(inside) else hi_
        nxt = not len(inside) and x < n
        crossed = False
        over, step, run2 = -1, -1, False
        if x >= n:
            q, kx = n, -1
        else:
            kx = int(k[x])
            over, step = int(F[x]) - target, int(e[x - 1])
            assert over in (0, 1) and step in (1, 2) and over < step
            run2 = bool(new[x] and x + 1 < n and a[x + 1] == a[x])
            if nxt:                               # derived from the run start carried into the next tile
                assert a[x] != a[x - 1] or kx == (x - (int(carry[tile + 1]) - 1)) % 255
            q = x
            if kx:
                q, kk = x + 1, kx + 1
                while q < n and kk < 255 and a[q] == a[x]:
                    q, kk = q + 1, kk + 1
                crossed = min(q, n - 1) // T > x // T
        blocks.append(Block(start, q, "search", 0, 0, x, kx, nxt, bool(nxt and a[x] != a[x - 1]), x >= n, crossed, False,
                            why, int(F[q]) - f_start, over, step, run2))
        start, f_start = q, int(F[q])
    assert start == n, "the mirrored chain ran out of block slots"
    want = rule_bounds(k, F, n, level)
    assert [(b.lo, b.hi) for b in blocks] == [(lo, hi) for lo, hi, _ in want], "the mirrored chain disagrees with the rule"

    ev_p = np.flatnonzero(e == 2)
    ps = np.flatnonzero(k == 0)
    pe = np.append(ps[1:], n)
    pi = np.searchsorted(ps, ev_p, "right") - 1
    extra = pe[pi] - ps[pi] - 4
    reach = np.minimum(ev_p + extra + (extra < 251), n - 1)      # the last byte the look-ahead reads
    ends = np.array([b.hi for b in blocks])
    return Trace(n, nt, flag_a, flag_b, carry, own_rs, blocks, refusals, ev_p, extra, reach // T > ev_p // T,
                 np.isin(ev_p + 1, ends) & (extra == 0), scan_shape(nt, scan_seg),
                 [(b.lo % 16, b.hi - b.lo, (b.hi - b.lo) % 16 != 0) for b in blocks])


# ---------------------------------------------------------------- builders

def plain(n, seed=1):
    """n bytes below 200 with no two equal neighbours: a walk whose steps are 1..199 (mod 200), the steps from a
    multiplicative hash of the index."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed * 7919)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    step = h % np.uint64(199) + np.uint64(1)
    return (np.cumsum(step) % np.uint64(200)).astype(np.uint8)


def put(a, pos, length, byte=200):
    """A run of `length` bytes (value >= 200, so neither neighbour in plain filler equals it) at pos."""
    assert byte >= 200 and 0 <= pos and pos + length <= len(a)
    assert (pos == 0 or a[pos - 1] != byte) and (pos + length == len(a) or a[pos + length] != byte)
    a[pos:pos + length] = byte
    return a


def runs_at(n, spots, seed=1):
    """Plain filler of n bytes with runs (pos, length) planted, their bytes 200, 201, ... in turn."""
    a = plain(n, seed)
    for i, (pos, length) in enumerate(spots):
        put(a, pos, length, 200 + i % 56)
    return a.tobytes()


def mixed(n, seed=1):
    """Plain filler with a run of 2..9, 255..259 or 300 bytes every 700 bytes or so, up to the last byte."""
    a = plain(n, seed)
    lens = (2, 3, 4, 5, 6, 9, 255, 256, 259, 300, 7, 4)
    pos, i = 37, 0
    while pos < n:
        put(a, pos, min(lens[i % len(lens)], n - pos), 200 + i % 56)
        pos += lens[i % len(lens)] + 331 + 97 * (i % 5)
        i += 1
    return a.tobytes()


def squeezed(pos, deficit, seed=1):
    """Filler of `pos` bytes whose RLE1 length is pos - deficit: runs of 255 (each swallows 250) and one shorter run
    from position 1000 on, 50 bytes apart; checked against the model."""
    a = plain(pos, seed)
    at, i = 1000, 0
    left = deficit
    while left > 0:
        ln = 255 if left >= 250 else left + 5
        put(a, at, ln, 200 + i % 56)
        left -= ln - 5
        at += ln + 50
        i += 1
    assert at < pos - 1000 and model(a)[4][pos] == pos - deficit
    return a


class Case(NamedTuple):
    build: object
    level: int = 1
    emu: bool = True
    big: bool = False
    size: int = 0       # big cases: the length, so that the scan shape is known without building them


CASES, GROUPS = {}, {}


def _add(group, name, build, level=1, emu=True, big=False, size=0):
    assert name not in CASES
    CASES[name] = Case(build, level, emu, big, size)
    GROUPS.setdefault(group, []).append(name)


# ---- pieces
_add("pieces", "tiny_1_l1", lambda: b"\x07")
_add("pieces", "tiny_1_l9", lambda: b"\x07", 9)
_add("pieces", "tiny_2_l9", lambda: b"ab", 9)
_add("pieces", "tiny_33_l1", lambda: plain(33).tobytes())
RUN_LENGTHS = list(range(1, 7)) + list(range(254, 261)) + list(range(509, 513)) + [768, 769, 770]
for _L in RUN_LENGTHS:
    _add("pieces", f"run{_L}_whole", lambda L=_L: bytes([201]) * L)
    _add("pieces", f"run{_L}_start", lambda L=_L: runs_at(L + 77, [(0, L)]))
    _add("pieces", f"run{_L}_end", lambda L=_L: runs_at(L + 77, [(77, L)]))          # (run4_end: a count of 0 ends the input)
    _add("pieces", f"run{_L}_twice", lambda L=_L: runs_at(2 * L + 90, [(40, L), (40 + L, L)]))

# ---- lane and tile edges
_add("edges", "lane_edge_run4", lambda: runs_at(3 * T, [(T + 64 * (d + 5) + d - 4, 4) for d in range(-3, 4)]))
for _d in range(-3, 4):
    # the run's last byte is at edge - 1 + d: d = 0 ends on the tile's last byte, d = 1..3 ends inside the next tile
    _add("edges", f"tile01_run4_{_d:+d}", lambda d=_d: runs_at(2 * T + 100, [(T + d - 4, 4)]))
    _add("edges", f"tile12_run4_{_d:+d}", lambda d=_d: runs_at(3 * T + 100, [(2 * T + d - 4, 4)]))
_add("edges", "run3_straddle", lambda: runs_at(3 * T + 50, [(T - 1, 3), (2 * T - 2, 3)]))
# a run of 258 whose 255 cut falls on the edge of tiles 1/2: four equal bytes end in tile 2 (kernel A flags it), but its
# three bytes of the run have k = 0, 1, 2 (kernel B clears the flag)
_add("edges", "cut_at_tile_edge", lambda: runs_at(3 * T + 100, [(2 * T - 255, 258)]))
_add("edges", "fourth_at_tile_end", lambda: runs_at(3 * T, [(T - 4, 4), (2 * T - 4, 10)]))
_add("edges", "look251_cross", lambda: runs_at(3 * T, [(2 * T - 100, 255), (T - 3, 255)]))
_add("edges", "longrun_from_8191", lambda: runs_at(6 * T, [(T - 1, 3 * T + 2 + 40)]))
_add("edges", "longrun_from_0", lambda: runs_at(6 * T, [(T, 3 * T + 5)]))
for _n in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
    _add("edges", f"len_{_n}", lambda n=_n: mixed(n, n))
_add("edges", "len_mod32_1", lambda: mixed(T + 32 * 5 + 1, 3))
_add("edges", "len_mod32_31", lambda: mixed(T + 32 * 9 + 31, 4))
_add("edges", "last_tile_1_continues", lambda: runs_at(2 * T + 1, [(2 * T - 4, 5)]))
_add("edges", "last_tile_1_starts", lambda: runs_at(2 * T + 1, [(2 * T - 6, 6)]))     # (the last byte is filler: a new run)


# ---- block-full edges
def _fit(total):
    """An input whose RLE1 length is `total`: a 4-run at 100 (five bytes), the rest plain."""
    return runs_at(total - 1, [(100, 4)])


def _full(k_at_x, run_len, tail=5000, level=1):
    """Block 0 fills at position x = nmax, which has k = k_at_x in a run of run_len bytes; the prefix is plain."""
    x = nmax(level)
    return runs_at(x - k_at_x + run_len + tail, [(x - k_at_x, run_len)])


for _d in (-1, 0, 1):
    _add("full", f"fit_nmax{_d:+d}", lambda d=_d: _fit(N1 + d))
_add("full", "fit_2nmax", lambda: _fit(2 * N1))
_add("full", "full_plain", lambda: runs_at(N1 + 5000, [(100, 4)]))                      # F = p + 1 behind the run: x is plain
_add("full", "full_k0", lambda: _full(0, 10))
_add("full", "full_k1", lambda: _full(1, 10))                                          # n = nmax + 4
_add("full", "full_k2", lambda: _full(2, 10))
_add("full", "full_k3", lambda: _full(3, 10))                                          # n = nmax + 2
_add("full", "full_step_tm1", lambda: runs_at(N1 + 5000, [(N1 - 4, 4)]))                # F: nmax - 1 -> nmax + 1
_add("full", "full_step_tm2", lambda: runs_at(N1 + 5000, [(N1 - 5, 4)]))                # F: nmax - 2 -> nmax
_add("full", "full_swallowed", lambda: runs_at(N1 + 5000, [(N1 - 4, 100)]))             # x = 5th byte of a 100-run
_add("full", "full_cut_255", lambda: _full(1, 255))                                     # the piece's last byte has k = 254
_add("full", "full_cut_256", lambda: _full(1, 256))                                     # the next block: one byte of the same run
_add("full", "full_cut_300", lambda: _full(1, 300))
_add("full", "full_cut_600", lambda: _full(2, 600))
_add("full", "full_piece_to_len", lambda: _full(1, 10, tail=0))


def _next_tile(run_back, run_len):
    """x is the first byte of tile 13: F(13 T) = nmax exactly (the filler before it swallows 13 T - nmax bytes), and a
    run starts run_back bytes before x (0: x starts a run of its own)."""
    X = 13 * T
    a = squeezed(X + 3000, X - N1)
    put(a, X - run_back, run_len, 255)
    b = a.tobytes()
    new, rs, k, e, F = model(a)
    assert F[X] == N1 and F[X - 1] < N1
    return b


_add("full", "x_next_tile_newrun", lambda: _next_tile(0, 7))
_add("full", "x_next_tile_plain", lambda: _next_tile(0, 1))
_add("full", "x_next_tile_k1", lambda: _next_tile(1, 9))
_add("full", "x_next_tile_k2", lambda: _next_tile(2, 300))


def _piece_cross():
    X = 13 * T - 6                               # x, k = 1, in a run of 20 that crosses the edge of tiles 12/13
    a = squeezed(X + 3000, X - N1)
    put(a, X - 1, 20, 255)
    assert model(a)[4][X] == N1
    return a.tobytes()


_add("full", "piece_end_cross_tile", _piece_cross)
_add("full", "block_nmax4_l9", lambda: _full(1, 40, tail=100, level=9), 9)
_add("full", "dense4", lambda: np.repeat((np.arange(40000) % 50 + 200).astype(np.uint8), 4).tobytes())


# ---- chain paths
def _drift():
    """65 plain blocks and more; a 3-run around each of the first 40 predicted boundaries (x has k = 1, the block ends
    two bytes later), placed one after the other from the boundary the model reports for the prefix."""
    a = plain(66 * N1 + 1000, 5)
    start, planned = 0, []
    for i in range(40):
        x = start + N1
        put(a, x - 1, 3, 200 + i % 56)
        start = x + 2
        planned.append(start)
    assert [hi for lo, hi, _ in rule_bounds(*_kF(a), 1)][:40] == planned
    return a.tobytes()


def _kF(a):
    new, rs, k, e, F = model(a)
    return k, F, len(a)


_add("chain", "batch_J2", lambda: plain(3 * N1 + 300, 2).tobytes())
_add("chain", "batch_J3", lambda: runs_at(4 * N1 + 300, [(N1 - 1, 2), (2 * N1, 3)], 3))
_add("chain", "batch_J64", lambda: plain(66 * N1 + 1000, 4).tobytes(), emu=False)
_add("chain", "batch_drift", _drift, emu=False)
_add("chain", "batch_refused", lambda: runs_at(4 * N1 + 300, [(3 * N1 + 50000, 4)], 6))
for _d in range(5):
    _add("chain", f"fast_refused_{_d}", lambda d=_d: plain(N1 + 4 - d, 7 + d).tobytes())
_add("chain", "fast_taken", lambda: plain(N1 + 5, 12).tobytes())
_add("chain", "last_not_plain", lambda: runs_at(N1 + 30000, [(N1 + 29000, 9)], 13))
_add("chain", "flag_at_start", lambda: runs_at(2 * N1 + 20000, [(0, 4)], 14))
_add("chain", "flag_at_end", lambda: runs_at(2 * N1 + 20000, [(2 * N1 + 20000 - 4, 4)], 15))


def _alternating():
    """Blocks 0, 2 and 4 plain, blocks 1 and 3 with runs in their middle only: the tiles that hold the boundaries are
    plain tiles, shared by a block that is read in place and one that is scattered.  The runs of block 3 are planted
    behind the boundaries the model reports for what precedes them."""
    a = plain(4 * N1 + 30000, 16)
    for i in range(6):
        put(a, N1 + 30000 + 5000 * i, (4, 5, 255, 256, 300, 700)[i], 200 + i)
    ends = [hi for lo, hi, _ in rule_bounds(*_kF(a), 1)]
    for i in range(6):
        put(a, ends[2] + 30000 + 5000 * i, (700, 4, 260, 6, 255, 510)[i], 210 + i)
    return a.tobytes()


_add("chain", "alternating", _alternating)


# ---- scans
def _scan(ntiles, ragged=0):
    """ntiles tiles of filler: the last run start of the first 16 tiles is in tile 15, and its run reaches three tiles
    into the next segment of the emulator's scans; a run of 300 across a tile edge of the last segment (its 255 cut
    hangs on the carry); short runs elsewhere."""
    n = ntiles * T - ragged
    return runs_at(n, [(16 * T - 100, 3 * T + 100), (5 * T - 2, 6), ((ntiles - 2) * T - 150, 300), (n - 9, 9)], ntiles)


_add("scans", "scan_32_tiles", lambda: _scan(32))
_add("scans", "scan_33_tiles", lambda: _scan(33, T - 1))           # two levels; the last segment is one tile of one byte
_add("scans", "scan_43_tiles", lambda: _scan(43, 1234))


def _big(ntiles):
    """Zeros at level 9 (2 to 4 blocks, cheap for the oracle): a run start planted in tile 8191, a stretch of whole
    tiles behind it that lives off the carry, a few more planted bytes, the last tile one byte long."""
    n = (ntiles - 1) * T + 1
    a = bytearray(n)
    for p in (8191 * T + 4000, 100, 5 * T - 1, 5 * T, n - 300, n - 2):
        a[p] = 1 + p % 200
    return bytes(a)


for _nt in (8193, 16384, 16385):
    _add("scans", f"scan_big_{_nt}", lambda nt=_nt: _big(nt), 9, emu=False, big=True, size=(_nt - 1) * T + 1)

# ---- CRC
CRC_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 65535, 65536, 65537, 131071, 131073)
for _n in CRC_LENGTHS:
    _add("crc", f"crc_{_n}", lambda n=_n: mixed(n, n % 97), 9)
_add("crc", "crc_17_blocks", lambda: plain(17 * N1, 17).tobytes(), emu=False)

NAMES = list(CASES)
BIG = "scan_big_8193"
AFTER_BIG = ["tiny_1_l1", "tiny_2_l9", "run4_whole", "run255_whole", "run5_end", "crc_17"]

_data = {}


def data(name):
    """The case's input, built once."""
    if name not in _data:
        d = CASES[name].build()
        assert isinstance(d, bytes) and d
        assert not CASES[name].size or len(d) == CASES[name].size, name       # (the scan shape the coverage test claims)
        _data[name] = d
    return _data[name]
