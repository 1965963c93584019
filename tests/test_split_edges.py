"""The first stage -- RLE1, the block splitter and the block CRCs (bzx_rle1.hip, bzx_rle1.h), their segmented copy in
bzx_batch.hip and the chunked entry bzx_split_rle1_chunk -- on inputs built to put its data-dependent paths on lane,
tile, block, segment and 16-byte edges (tests/split_cases.py): pieces of every length around the 4-byte and 255-byte
rules, runs around lane and tile edges, the block filled at every place a piece can be in, the three ways the chain
finds a boundary, the scans around two segments, CRC ranges around 16 bytes and 64 KiB.

split_cases.trace() mirrors the kernels' path decisions, and test_case_list_covers_the_edges proves from it that the
cases reach what they are named after.  split_cases.reference(), a whole-array numpy model of libbz2's rule with zlib's
CRC behind a bit reversal, is held against the oracle on every case that is not `big`: that licenses the oracle as
the expected value.  bzx_split_rle1 is then held against the oracle through the emulator (-m "not gpu") and on the
device (-m gpu); the chunked entry, the batched splitter, the sharded scatter with two and three ranks and the
decoder's use of the CRC kernel run on the same inputs, and test_gpu_largest_block_end_to_end holds bzx_compress_buffer
against bz2.compress on the level-9 input whose first block has nmax + 4 = 899,985 bytes.  Everything is equality."""
import bz2
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import split_cases as S
from bzx_cindex_ctypes import ENTRY, CIndexLib
from bzx_ctypes import EMU_PATH, ROOT, BzxLib

NAMES = S.NAMES
EMU_NAMES = [n for n in NAMES if S.CASES[n].emu]
SMALL = [n for n in NAMES if not S.CASES[n].big]
CSRC = os.path.join(ROOT, "bzip2-rust_amd", "csrc")
_cache = {}


def _emu_built():
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")]
    if not os.path.exists(EMU_PATH) or any(os.path.getmtime(s) > os.path.getmtime(EMU_PATH) for s in srcs):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "emu", "build_emu.sh")])


@pytest.fixture(scope="module")
def emu():
    _emu_built()
    lib = BzxLib(EMU_PATH)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def emu_batch():
    _emu_built()
    lib = CIndexLib(EMU_PATH, max_blocks=16)
    yield lib
    lib.close()


@pytest.fixture(scope="module")
def gpu_batch():
    lib = CIndexLib(max_blocks=64)
    yield lib
    lib.close()


def _want(oracle, name):
    """The oracle's blocks of the case, [(image, crc)]: computed once."""
    if ("want", name) not in _cache:
        _cache["want", name] = oracle.split_rle1(S.data(name), S.CASES[name].level)
    return _cache["want", name]


def _reference(name):
    if ("ref", name) not in _cache:
        _cache["ref", name] = S.reference(S.data(name), S.CASES[name].level)
    return _cache["ref", name]


def _trace(name, seg=S.SCAN_SEG):
    if ("trace", name, seg) not in _cache:
        _cache["trace", name, seg] = S.trace(S.data(name), S.CASES[name].level, seg)
    return _cache["trace", name, seg]


def _bz2(name_or_bytes, level=1):
    key = ("bz2", name_or_bytes, level)
    if key not in _cache:
        d = S.data(name_or_bytes) if isinstance(name_or_bytes, str) else name_or_bytes
        _cache[key] = bz2.compress(d, level)
    return _cache[key]


def _split(lib, data, level, nblk_cap):
    """bzx_split_rle1 -> [(image, crc)].  The slabs start out as 0xA5 so that a count byte the stage never wrote cannot
    pass for a count of 0; nblk_cap slabs only (the big cases have a handful of blocks)."""
    slabs = C.create_string_buffer(nblk_cap * S.MAX_BLOCK)
    C.memset(slabs, 0xA5, nblk_cap * S.MAX_BLOCK)
    ns, crcs, nb = (C.c_uint32 * nblk_cap)(), (C.c_uint32 * nblk_cap)(), C.c_uint32()
    lib._check(lib.lib.bzx_split_rle1(lib.ctx, data, len(data), level, slabs, nblk_cap, ns, crcs, C.byref(nb)))
    return [(C.string_at(C.addressof(slabs) + b * S.MAX_BLOCK, ns[b]), crcs[b]) for b in range(nb.value)]


def _split_case(lib, oracle, name):
    return _split(lib, S.data(name), S.CASES[name].level, len(_want(oracle, name)) + 1)


def _split_chunks(lib, data, level, pieces):
    """bzx_split_rle1_chunk over pieces of the given lengths (zeros are empty calls; the last call is the final one)."""
    L = lib.lib
    L.bzx_split_rle1_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_uint32,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    assert sum(pieces) == len(data)
    capb = 4
    buf = C.create_string_buffer(capb * S.MAX_BLOCK)
    ns, crcs, nb = (C.c_uint32 * capb)(), (C.c_uint32 * capb)(), C.c_uint32()
    out, off = [], 0
    for i, n in enumerate(pieces):
        C.memset(buf, 0xA5, capb * S.MAX_BLOCK)
        lib._check(L.bzx_split_rle1_chunk(lib.ctx, data[off:off + n], n, level, int(i == len(pieces) - 1), buf, capb, ns, crcs,
                                          C.byref(nb)))
        out += [(C.string_at(C.addressof(buf) + b * S.MAX_BLOCK, ns[b]), crcs[b]) for b in range(nb.value)]
        off += n
    return out


def _chunk_plan(name):
    """Piece lengths of a chunked run of the case, from the reference's boundaries q: borders at q - 2 .. q + 2 (so
    one-byte chunks across every boundary, borders at q - 1, q, q + 1); behind the 4th byte of a piece and at k = 254
    and k = 255 of a run, each at the first such places of the input and at the two nearest before and behind every q
    (where the carry of the chunked entry meets the end of a block); an empty call behind the first piece and an empty
    final call."""
    d = S.data(name)
    a = np.frombuffer(d, dtype=np.uint8)
    new, rs, k, e, F = S.model(a)
    fourth, k254 = np.flatnonzero(e == 2), np.flatnonzero(k == 254)

    def near(ps, q):
        i = int(np.searchsorted(ps, q))
        return [int(p) for p in ps[max(i - 2, 0):i + 2]]

    cuts = set()
    at4, at254 = [int(p) for p in fourth[:3]], [int(p) for p in k254[:2]]
    for _, _, _, hi in _reference(name):
        cuts.update(range(hi - 2, hi + 3))
        at4 += near(fourth, hi)
        at254 += near(k254, hi)
    cuts.update(p + 1 for p in at4)
    for p in at254:
        cuts.update((p, p + 1))
    cuts = sorted(c for c in cuts if 0 < c < len(d))
    edges = [0] + cuts + [len(d)]
    pieces = [b - a_ for a_, b in zip(edges, edges[1:])]
    return pieces[:1] + [0] + pieces[1:] + [0]


def _chunked_ok(lib, oracle, name):
    assert _split_chunks(lib, S.data(name), S.CASES[name].level, _chunk_plan(name)) == _want(oracle, name), name


def _same_run(n):
    """Two inputs of n bytes that end and begin in the same byte run of 300 bytes."""
    pair = (S.runs_at(n, [(n - 300, 300)]), S.runs_at(n, [(0, 300)]))
    assert pair[0][-300:] == pair[1][:300] and pair[0][-301] != pair[0][-300]
    return pair


def _batch_inputs(names, pair):
    """The cases in order with an empty input after every fifth, and the pair that shares a byte run side by side."""
    inputs = []
    for i, name in enumerate(names):
        inputs.append(S.data(name))
        if i % 5 == 4:
            inputs.append(b"")
    mid = len(inputs) // 2
    return inputs[:mid] + list(pair) + inputs[mid:] + [b""]


def _batch_ok(lib, names, pair, both_orders):
    """One bzx_compress_batch_buffer call at level 1 with index keeping on, in list order (and reversed): stream i is
    libbz2's, and the index entries' decoded lengths are the raw lengths of the reference's blocks."""
    assert lib.keep_index(1) == 0
    for inputs in (_batch_inputs(names, pair), _batch_inputs(names, pair)[::-1])[:2 if both_orders else 1]:
        streams = lib.batch_buffer(inputs, 1)
        rc, slices = lib.batch_get_index()
        assert rc == 0 and len(slices) == len(inputs) == len(streams)
        for i, d in enumerate(inputs):
            assert streams[i] == _bz2(d), (i, len(d))
            got = [ENTRY.unpack_from(slices[i], 40 * j)[2] for j in range(len(slices[i]) // 40)]
            assert got == S.raw_lengths(d, 1), (i, len(d))


def _dirty_sequence(lib, oracle):
    assert _split_case(lib, oracle, S.BIG) == _want(oracle, S.BIG)
    for name in S.AFTER_BIG:
        assert _split_case(lib, oracle, name) == _want(oracle, name), name


# ---------------------------------------------------------------- CPU

def test_constants_match_the_sources():
    """The constants mirrored in split_cases.py are those of the sources and of the emulator build."""
    def read(*p):
        with open(os.path.join(ROOT, *p)) as f:
            return f.read()
    env = S.parse_constants(read("bzip2-rust_amd", "csrc", "bzx_rle1.h"), read("bzip2-rust_amd", "csrc", "bzx_rle1.hip"),
                            read("tests", "emu", "build_emu.sh"))
    for name in ("RL_NT", "RL_BYTES", "RL_TILE", "BND_J", "BND_W", "CRC_TILE", "SCAN_SEG", "SCAN_SEG_EMU"):
        assert env[name] == getattr(S, name), name
    assert S.crc_bzip2(b"123456789") == 0xFC891918
    assert S.N1 == 99981 and S.N1 % 16 == 13


def _case_edges(name):
    """The edges the case reaches, from trace(): a set of labels."""
    c = S.CASES[name]
    if c.big:
        # (never built here: their scan shape follows from their length alone, which data() checks on the device)
        return {("device scan", S.scan_shape(-(-c.size // S.T), S.SCAN_SEG))}
    got = set()
    hit = got.add
    t = _trace(name)
    d = S.data(name)
    bl = t.blocks
    # ---- pieces
    if t.n <= 2:
        hit(("tiny", c.level))
    if len(set(d)) == 1:
        hit(("whole run", t.n))
    if len(t.ev_p):
        for x in set(t.ev_extra.tolist()) & {0, 1, 2, 250, 251}:
            hit(("count", x))
        if t.ev_p[-1] == t.n - 1:
            hit("4-run ends the input")
        if (t.ev_p % 32 == 31).any():
            hit("two-byte write on a lane's last byte")
        if (t.ev_p % S.T == S.T - 1).any():
            hit("two-byte write on a tile's last byte")
        if t.ev_block_end.any():
            hit("two-byte write ends a block")
        if (t.ev_cross & (t.ev_extra == 251)).any():
            hit("251-byte look-ahead across a tile edge")
    # ---- tiles
    if (t.flag_a[1:t.n // S.T] & ~t.flag_b[1:t.n // S.T]).any():         # (whole inner tiles: A tests only those)
        hit("A flags a tile that B clears")
    for ti in range(1, t.ntiles):
        if not t.own_rs[ti] and ti + 1 < t.ntiles and not t.own_rs[ti + 1] and t.carry[ti] % S.T in (0, 1):
            hit(("tiles without a run start, run from tile offset", int(t.carry[ti] - 1) % S.T))
    if t.n % 32 in (1, 31) and t.n > S.T:
        hit(("len % 32", t.n % 32))
    if t.n % S.T == 1 and t.n > S.T:
        hit(("one-byte last tile", "starts a run" if d[-1] != d[-2] else "continues a run"))
    if t.n in (S.T - 1, S.T, S.T + 1, 2 * S.T, 2 * S.T + 1):
        hit(("len", t.n))
    # ---- blocks
    for i, b in enumerate(bl):
        if b.path == "batch":
            hit(("batch J", b.J))
            if b.woff >= 64:
                hit("window offset >= 64")
        if b.path == "single":
            hit("single fast path")
        if b.refused.startswith("len:"):
            hit(("single refused by the end of the input", int(b.refused[4:])))
        if b.path == "search":
            hit(("search, k at x", b.k_x))
            if not b.x_ge_len:
                # where the target was reached: F(x) - target, what the byte before x emitted, and what x is
                at = "k = %d" % b.k_x if b.k_x else "a run start" if b.x_run2 else "a plain byte"
                hit(("filled",) + _filled(b.over, b.step, at))
            if b.x_next_tile:
                hit(("x is a next tile's first byte", "new run" if b.x_newrun else "continued run k=%d" % b.k_x))
            if b.x_ge_len:
                hit("x >= len")
            if b.end_crossed:
                hit("piece end across a tile edge")
            if b.hi == t.n and b.k_x > 0:
                hit("the filling piece ends the input")
            if b.k_x > 0 and b.hi - (b.x - b.k_x) == 255 and b.hi < t.n and d[b.hi] == d[b.hi - 1]:
                hit("next block starts behind a 255 cut in the same run")
            if b.k_x > 0 and b.hi - (b.x - b.k_x) == 255 and (b.hi == t.n or d[b.hi] != d[b.hi - 1]):
                hit("the filling piece is a whole run of 255")
        if b.n == S.nmax(c.level) + 4:
            hit(("block of nmax + 4", c.level))
        if b.path == "last":
            hit(("last block", "plain" if b.plain else "not plain"))
        if i and bl[i - 1].plain != b.plain and b.lo % S.T and not t.flag_b[b.lo // S.T]:
            hit("a plain tile and a lane hold the border of a plain and a non-plain block")
    if t.batch_refused and any(b.path == "single" for b in bl):
        hit("batch refused by a flagged tile")
    if all(b.plain for b in bl) and len(bl) >= 2:
        hit("every block read in place")
    flagged = np.flatnonzero(t.flag_b)
    if len(flagged) == 1 and len(bl) >= 2:
        hit(("one flagged tile", "start" if flagged[0] == 0 else "end" if flagged[0] == t.ntiles - 1 else "inside"))
    kinds = [b.plain for b in bl]
    if len(bl) >= 4 and all(kinds[i] != kinds[i + 1] for i in range(len(bl) - 1)):
        hit("plain and non-plain blocks in turn")
    f_len = sum(b.n for b in bl)
    for m, lab in ((S.nmax(c.level) - 1, "nmax-1"), (S.nmax(c.level), "nmax"), (S.nmax(c.level) + 1, "nmax+1"),
                   (2 * S.nmax(c.level), "2nmax")):
        if f_len == m:
            hit(("RLE1 length", lab, len(bl)))
    if f_len * 4 == t.n * 5 and len(bl) >= 2:
        hit(("densest", S.max_blocks(t.n, c.level) - len(bl)))
    # ---- scans of the emulator build
    if c.emu:
        levels, _, nseg, last = S.scan_shape(t.ntiles, S.SCAN_SEG_EMU)
        if t.ntiles >= 32 and t.own_rs[15] and not t.own_rs[16] and t.carry[16] > 15 * S.T:
            hit(("emu scan", t.ntiles, levels, nseg, last))
    # ---- CRC
    if len(bl) == 1:
        hit(("crc length", t.n))
    if len({lo16 for lo16, _, _ in t.crc}) == 16:
        hit("crc block starts on all 16 residues")
    if any(partial for _, _, partial in t.crc):
        hit("crc partial piece")
    return got


def _edges(names):
    """The edges the named cases reach; ("emu", label) where a case that runs through the emulator reaches it."""
    got = set()
    for name in names:
        if name not in _cache.setdefault("edges", {}):
            _cache["edges"][name] = _case_edges(name)
        labels = _cache["edges"][name]
        got |= labels
        if S.CASES[name].emu:
            got |= {("emu", lab) for lab in labels}
    return got


def _filled(over, step, at):
    return ("F(x) - target = %d" % over, "by a step of %d" % step, "at " + at)


FILLED_AT = {
    "full_plain": _filled(0, 1, "a plain byte"), "full_k0": _filled(0, 1, "a run start"), "full_k1": _filled(0, 1, "k = 1"),
    "full_k2": _filled(0, 1, "k = 2"), "full_k3": _filled(0, 1, "k = 3"), "full_step_tm1": _filled(1, 2, "a plain byte"),
    "full_step_tm2": _filled(0, 2, "a plain byte"), "full_swallowed": _filled(1, 2, "k = 4"),
}


def _required():
    need = set()
    plain_labels = [
        ("tiny", 1), ("tiny", 9), "4-run ends the input", ("count", 0), ("count", 251), ("count", 250),
        "two-byte write on a lane's last byte", "two-byte write on a tile's last byte", "two-byte write ends a block",
        "251-byte look-ahead across a tile edge", "A flags a tile that B clears",
        ("tiles without a run start, run from tile offset", S.T - 1), ("tiles without a run start, run from tile offset", 0),
        ("len % 32", 1), ("len % 32", 31), ("one-byte last tile", "starts a run"), ("one-byte last tile", "continues a run"),
        ("batch J", 2), ("batch J", 3), "single fast path", "batch refused by a flagged tile",
        ("x is a next tile's first byte", "new run"), ("x is a next tile's first byte", "continued run k=1"),
        ("x is a next tile's first byte", "continued run k=2"), "x >= len", "piece end across a tile edge",
        "the filling piece ends the input", "next block starts behind a 255 cut in the same run",
        "the filling piece is a whole run of 255", ("block of nmax + 4", 1), ("block of nmax + 4", 9),
        ("last block", "plain"), ("last block", "not plain"), "every block read in place",
        ("one flagged tile", "start"), ("one flagged tile", "end"), "plain and non-plain blocks in turn",
        "a plain tile and a lane hold the border of a plain and a non-plain block",
        ("RLE1 length", "nmax-1", 1), ("RLE1 length", "nmax", 1), ("RLE1 length", "nmax+1", 2), ("RLE1 length", "2nmax", 2),
        ("densest", 1), "crc partial piece",
    ]
    # where the block fills: at a plain byte, at k = 0 .. 3 by a one-byte step, over the two-byte step of a 4th byte from
    # target - 1 (F jumps the target) and from target - 2, inside the swallowed part of a piece
    plain_labels += [("filled",) + at for at in FILLED_AT.values()]
    plain_labels += [("whole run", L) for L in S.RUN_LENGTHS]
    plain_labels += [("len", n) for n in (S.T - 1, S.T, S.T + 1, 2 * S.T, 2 * S.T + 1)]
    plain_labels += [("search, k at x", k) for k in range(5)]
    plain_labels += [("single refused by the end of the input", dd) for dd in range(5)]
    plain_labels += [("crc length", n) for n in S.CRC_LENGTHS]
    for case, at in FILLED_AT.items():           # the block-full cases are what their names say
        assert ("filled",) + at in _case_edges(case), case
    for lab in plain_labels:                     # each of them through the emulator too
        need.add(lab)
        need.add(("emu", lab))
    # device only: J = 64, the window drift, the 16-residue CRC input, the three big scan shapes
    need |= {("batch J", 64), "window offset >= 64", "crc block starts on all 16 residues",
             ("device scan", (1, 2, 1, 8193)), ("device scan", (1, 2, 1, 16384)), ("device scan", (2, 1, 3, 1))}
    # the emulator's scans: 32 tiles on one level, 33 and 43 on two (the last segment one tile and eleven)
    need |= {("emu scan", 32, 1, 1, 32), ("emu scan", 33, 2, 3, 1), ("emu scan", 43, 2, 3, 11)}
    return need


def test_case_list_covers_the_edges():
    """From trace() over CASES: every edge the groups are named after is reached by a case, all but the six
    device-only ones by a case that runs through the emulator; without any one group something is lost.  The run
    cases are checked to be what their names say here, too."""
    assert sum(len(g) for g in S.GROUPS.values()) == len(NAMES)
    not_emu = [n for n in NAMES if not S.CASES[n].emu]
    assert len(not_emu) <= 8
    assert all((S.CASES[n].size or len(S.data(n))) > 1 << 20 for n in not_emu)
    assert all(S.CASES[n].emu for n in NAMES if not S.CASES[n].big and len(S.data(n)) <= 1 << 20)
    need = _required()
    got = _edges(NAMES)
    assert not need - got, sorted(map(str, need - got))
    for group, members in S.GROUPS.items():
        rest = _edges([n for n in NAMES if n not in members])
        assert need - rest, group
    # runs: every length, in the four positions, is the run its name says (and only that)
    for L in S.RUN_LENGTHS:
        for pos, nruns in (("whole", 1), ("start", 1), ("end", 1), ("twice", 2)):
            d = np.frombuffer(S.data(f"run{L}_{pos}"), dtype=np.uint8)
            runs = [int(x) for x in np.diff(np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1], [True])))) if x > 1 or L == 1]
            if L > 1:
                assert runs == [L] * nruns, (L, pos)
        assert S.data(f"run{L}_start")[0] >= 200 and S.data(f"run{L}_end")[-1] >= 200
    # 4-runs around the edges: each ends where its name says; the 3-runs leave both tiles plain
    ends = sorted(int(p) for p in _trace("lane_edge_run4").ev_p)
    assert [p % 32 for p in ends] == [(31 + d) % 32 for d in range(-3, 4)] and all(S.T <= p < 2 * S.T for p in ends)
    for d in range(-3, 4):
        assert _trace(f"tile01_run4_{d:+d}").ev_p.tolist() == [S.T - 1 + d]
        assert _trace(f"tile12_run4_{d:+d}").ev_p.tolist() == [2 * S.T - 1 + d]
    t = _trace("run3_straddle")
    assert not t.flag_a[1:3].any() and not t.flag_b.any() and len(t.ev_p) == 0
    # the filler has no two equal neighbours
    f = S.plain(300000, 9)
    assert (f[1:] != f[:-1]).all() and f.max() < 200


def test_reference_agrees_with_oracle(oracle):
    """The numpy model and the oracle agree on every case that is built here, in images and CRCs."""
    for name in SMALL:
        ref = _reference(name)
        assert [(img, crc) for img, crc, _, _ in ref] == _want(oracle, name), name
        assert ref[0][2] == 0 and ref[-1][3] == len(S.data(name)) and all(a[3] == b[2] for a, b in zip(ref, ref[1:]))


@pytest.mark.parametrize("name", EMU_NAMES)
def test_emu_case(emu, oracle, name):
    assert _split_case(emu, oracle, name) == _want(oracle, name)


EMU_CHUNKED = ["run260_twice", "full_cut_300", "tile12_run4_+0"]
# (tile01_run4_+2: the second input of the batch, so its tiles are 1 and 2 of the call, and its second tile starts at
# k = 2 of a run: the emission there hangs on the run start carried into the tile, which the batch keeps in the
# numbering of the whole call)
EMU_BATCH = ["tiny_1_l1", "tile01_run4_+2", "run4_end", "run255_whole", "run770_twice", "crc_17"]


def test_emu_chunked(emu, oracle):
    for name in EMU_CHUNKED:
        _chunked_ok(emu, oracle, name)


def test_emu_batch(emu_batch):
    _batch_ok(emu_batch, EMU_BATCH, _same_run(700), both_orders=False)


# ---------------------------------------------------------------- device

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_case(bzx, oracle, name):
    got = _split_case(bzx, oracle, name)
    assert got == _want(oracle, name)
    if not S.CASES[name].big:
        assert got == [(img, crc) for img, crc, _, _ in _reference(name)]      # (this one owes the oracle nothing)


@pytest.mark.gpu
def test_gpu_chunked(bzx, oracle):
    """bzx_split_rle1_chunk on the piece and block-full cases of at most 1 MB, cut where _chunk_plan says."""
    for name in S.GROUPS["pieces"] + S.GROUPS["full"]:
        if len(S.data(name)) <= 1_000_000:
            _chunked_ok(bzx, oracle, name)


@pytest.mark.gpu
def test_gpu_batch(gpu_batch):
    _batch_ok(gpu_batch, [n for n in SMALL if len(S.data(n)) <= 1_000_000], _same_run(5000), both_orders=True)


def _shard_ok(make_lib, device, name, worlds, scanned):
    """The protocol of tests/shard_worker.py with torch sums and copies in the place of the collectives: one context per
    rank in this process, one rank after the other.  The stream is libbz2's and every block is reported by its rank."""
    import torch
    level = 1
    d = S.data(name)
    want = _bz2(name)
    nblk_want = len(_reference(name))
    host = torch.zeros(len(d) + 16, dtype=torch.uint8)
    host = host[(-host.data_ptr()) % 16:][:len(d)]
    host.copy_(torch.frombuffer(bytearray(d), dtype=torch.uint8))
    raw = host.to(device)
    assert raw.data_ptr() % 16 == 0
    for world in worlds:
        libs = [make_lib() for _ in range(world)]
        try:
            L = libs[0].lib
            L.bzx_shard_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32,
                                            C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
            L.bzx_shard_emit_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_size_t)]
            L.bzx_shard_assemble_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            L.bzx_shard_assemble_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
            L.bzx_shard_scan_entries.restype = C.c_size_t
            L.bzx_shard_scan_entries.argtypes = [C.c_size_t, C.c_uint32]
            for f in (L.bzx_shard_scan_runs, L.bzx_shard_scan_counts):
                f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p]
            L.bzx_shard_prepare_scanned.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
            L.bzx_ctx_sync.argtypes = [C.c_void_p]

            def dev_sync():
                if device != "cpu":
                    torch.cuda.synchronize()

            def sync(lib):
                lib._check(L.bzx_ctx_sync(lib.ctx))
                dev_sync()

            bits = [torch.zeros(64, dtype=torch.int64, device=device) for _ in range(world)]
            nblk = [C.c_uint32() for _ in range(world)]
            dev_sync()
            if scanned:
                P = L.bzx_shard_scan_entries(len(d), world)
                tiles = [torch.full((3, world, P), -7, dtype=torch.int64, device=device) for _ in range(world)]
                dev_sync()
                for r, lib in enumerate(libs):
                    lib._check(L.bzx_shard_scan_runs(lib.ctx, raw.data_ptr(), len(d), r, world, tiles[r].data_ptr()))
                    sync(lib)
                for r in range(world):                       # the all-gather of array 0
                    for o in range(world):
                        tiles[o][0, r] = tiles[r][0, r]
                dev_sync()
                for r, lib in enumerate(libs):
                    lib._check(L.bzx_shard_scan_counts(lib.ctx, raw.data_ptr(), len(d), r, world, tiles[r].data_ptr()))
                    sync(lib)
                for a in (1, 2):
                    for r in range(world):
                        for o in range(world):
                            tiles[o][a, r] = tiles[r][a, r]
                dev_sync()
                for r, lib in enumerate(libs):
                    lib._check(L.bzx_shard_prepare_scanned(lib.ctx, raw.data_ptr(), len(d), level, r, world, tiles[r].data_ptr(),
                                                           C.byref(nblk[r]), bits[r].data_ptr(), 64))
                    sync(lib)
            else:
                for r, lib in enumerate(libs):
                    lib._check(L.bzx_shard_prepare(lib.ctx, raw.data_ptr(), len(d), level, r, world, C.byref(nblk[r]),
                                                   bits[r].data_ptr(), 64))
                    sync(lib)
            assert [n.value for n in nblk] == [nblk_want] * world
            # every block is reported by exactly one rank: its own
            owners = torch.stack([(b[:nblk_want] != 0) for b in bits]).to(torch.int64).cpu()
            assert owners.sum(dim=0).tolist() == [1] * nblk_want
            assert all(int(owners[b % world, b]) == 1 for b in range(nblk_want))
            total = torch.stack(bits).sum(dim=0)
            dev_sync()
            cap = len(d) + 65536
            packed, plen = [], []
            sl = C.c_size_t()
            for r, lib in enumerate(libs):
                p = torch.zeros(cap // 4, dtype=torch.int32, device=device)
                dev_sync()
                pl = C.c_size_t()
                lib._check(L.bzx_shard_emit_packed(lib.ctx, total.data_ptr(), p.data_ptr(), cap, C.byref(pl), C.byref(sl)))
                sync(lib)
                assert pl.value % 4 == 0
                packed.append(p)
                plen.append(pl.value)
            out = torch.full((cap // 4,), -1, dtype=torch.int32, device=device)      # assemble_begin must clear what it uses
            dev_sync()
            ol = C.c_size_t()
            libs[0]._check(L.bzx_shard_assemble_begin(libs[0].ctx, out.data_ptr(), cap, C.byref(ol)))
            assert ol.value == sl.value
            for r in range(world):
                libs[0]._check(L.bzx_shard_assemble_rank(libs[0].ctx, packed[r].data_ptr(), r, out.data_ptr()))
            sync(libs[0])
            assert out.cpu().numpy().tobytes()[:ol.value] == want, (world, scanned)
        finally:
            for lib in libs:
                lib.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scanned", [False, True])
def test_gpu_shard_worlds_on_one_device(scanned):
    """The sharded scatter with two and three ranks on the device (own_step > 1: the blocks of other ranks and the plain
    blocks are passed over lane by lane), with bzx_shard_prepare and with the scan_runs / scan_counts / prepare_scanned
    form, on the input whose blocks are plain and non-plain in turn."""
    _shard_ok(lambda: BzxLib(max_blocks=16), "cuda", "alternating", (2, 3), scanned)


@pytest.mark.gpu
def test_gpu_decode_crc(bzx):
    """bzx_launch_block_crcs, the decoder's use of the CRC kernel, on ranges of the same lengths: the decoder verifies
    every block's CRC on the device and returns the bytes."""
    for name in S.GROUPS["crc"] + S.GROUPS["pieces"]:
        d, level = S.data(name), S.CASES[name].level
        assert bzx.decompress_buffer(_bz2(name, level), cap=len(d) + 64) == d, name


@pytest.mark.gpu
def test_gpu_largest_block_end_to_end(bzx):
    """block_nmax4_l9 through bzx_compress_buffer at level 9: its first block has 899,985 bytes, the largest the stages
    behind the splitter ever see, and the stream is libbz2's."""
    assert [len(img) for img, _, _, _ in _reference("block_nmax4_l9")][0] == S.nmax(9) + 4 == 899_985
    assert bzx.compress_buffer(S.data("block_nmax4_l9"), 9) == _bz2("block_nmax4_l9", 9)


@pytest.mark.gpu
def test_gpu_dirty_context(bzx, oracle):
    """The 64 MiB case, then the smallest ones on the same context: tile arrays, segment totals and slabs that the big
    input left behind must not show."""
    _dirty_sequence(bzx, oracle)


@pytest.mark.gpu
def test_gpu_cases_back_to_back(bzx, oracle):
    """Every case that is not big, then all of them in reverse order, on the one context, the levels changing between
    the calls."""
    for name in SMALL + SMALL[::-1]:
        assert _split_case(bzx, oracle, name) == _want(oracle, name), name
