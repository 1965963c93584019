"""ctypes bindings of the record layer (include/bzx.h: bzx_index_count_records, bzx_index_get_records,
bzx_index_build_records_buffer, bzx_records_*, bzx_decompress_records_*, bzx_stage_rec_*), used by the record tests, the
command-line test and the probe.  RecordsLib is the RangesLib of bzx_ranges_ctypes.py with those functions bound; the
host-only planners are also reachable without a context, through planners()."""
import ctypes as C
import struct

from bzx_ctypes import LIB_PATH
from bzx_range_ctypes import IndexEntry, IndexInfo
from bzx_ranges_ctypes import Piece, RangesLib, RangesResult, u64

U64P, U32P, SZP, INTP = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.POINTER(C.c_int)
NONE = 0xFFFFFFFF

BZXR_HEADER = struct.Struct("<4sIIIQQ")          # magic, version, delimiter, zero, nblk, T; 32 bytes
assert BZXR_HEADER.size == 32


def pack_bzxr(delim, table):
    """A record table -> the bytes of FILE.bz2.bzxr."""
    return BZXR_HEADER.pack(b"BZXR", 1, delim, 0, len(table) - 1, table[-1]) + struct.pack(f"<{len(table)}Q", *table)


def read_bzxr(path):
    """A stored record table -> (delimiter, [rec_before])."""
    with open(path, "rb") as f:
        raw = f.read()
    magic, version, delim, zero, nblk, total = BZXR_HEADER.unpack_from(raw)
    assert magic == b"BZXR" and version == 1 and zero == 0 and len(raw) == 32 + 8 * (nblk + 1)
    table = list(struct.unpack_from(f"<{nblk + 1}Q", raw, 32))
    assert table[-1] == total
    return delim, table


def u32(values):
    return (C.c_uint32 * max(len(values), 1))(*values)


def bind_planners(L):
    L.bzx_records_span.argtypes = [U64P, C.c_uint64, C.c_uint64, U64P, U64P]
    L.bzx_records_pieces.argtypes = [C.c_void_p, C.c_uint64, U64P, C.c_uint32, U64P, U64P, U64P, U64P, C.c_uint32, U32P]


class Planners:
    """bzx_records_span and bzx_records_pieces: host only, no context."""

    def __init__(self, lib):
        self.lib = lib
        bind_planners(lib)

    def span(self, table, r, n=None):
        """-> (rc, entry, j)"""
        n = len(table) - 1 if n is None else n
        entry, j = C.c_uint64(12345), C.c_uint64(12345)
        rc = self.lib.bzx_records_span(u64(table) if table is not None else None, n, r, C.byref(entry), C.byref(j))
        return rc, entry.value, j.value

    def pieces(self, entries, n, table, ranges, cap=None):
        """-> (rc, [(base, len)], pieces needed)"""
        cap = 2 * len(ranges) + 4 if cap is None else cap
        bases, lens, np = u64([0] * cap), u64([0] * cap), C.c_uint32(12345)
        rc = self.lib.bzx_records_pieces(entries, n, u64(table), len(ranges), u64([r[0] for r in ranges]),
                                         u64([r[1] for r in ranges]), bases, lens, cap, C.byref(np))
        return rc, [(bases[i], lens[i]) for i in range(min(cap, np.value))], np.value


def planners(path=LIB_PATH):
    return Planners(C.CDLL(path))


class RecordsLib(RangesLib, Planners):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        RangesLib.__init__(self, path, device, max_blocks)
        L = self.lib
        bind_planners(L)
        L.bzx_index_count_records.argtypes = [C.c_void_p, C.c_int]
        L.bzx_index_get_records.argtypes = [C.c_void_p, C.POINTER(U64P), U64P]
        L.bzx_index_build_records_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint64,
                                                     C.POINTER(IndexInfo), U64P]
        for fn in (L.bzx_records_count_device, L.bzx_records_count_buffer):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_uint64, U64P]
        for fn in (L.bzx_records_locate_device, L.bzx_records_locate_buffer):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, U64P, C.c_int, C.c_uint32, U64P, U64P, INTP]
        for fn in (L.bzx_decompress_records_device, L.bzx_decompress_records_buffer):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, U64P, C.c_int, C.c_uint32, U64P, U64P,
                           C.c_void_p, C.c_size_t, SZP, SZP, INTP, SZP]
        L.bzx_stage_rec_count.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, U64P, U64P, C.c_int, U32P]
        L.bzx_stage_rec_select.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, U64P, U64P, U32P, C.c_int, U32P, U32P]
        L.bzx_salvage_begin.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]

    # ---- the table
    def index_records(self, z, delim, cap=None):
        """bzx_index_build_records_buffer -> (rc, entries, info, [rec_before of the entries written])."""
        cap = len(z) // 32 + 64 if cap is None else cap
        entries, info, table = (IndexEntry * max(cap, 1))(), IndexInfo(), u64([0xA5A5] * (cap + 1))
        rc = self.lib.bzx_index_build_records_buffer(self.ctx, bytes(z), len(z), delim, entries, cap, C.byref(info), table)
        return rc, entries, info, list(table[:min(info.nblk, cap) + 1])

    def index_feed_records(self, z, delim, feeds=0, max_chunk=0):
        """bzx_index_* with counting over z in pieces of `feeds` bytes -> (rc, [entry keys], info, [rec_before])."""
        h = C.c_void_p()
        assert self.lib.bzx_index_begin(self.ctx, max_chunk, C.byref(h)) == 0, self.last_error()
        try:
            if delim is not None:
                assert self.lib.bzx_index_count_records(h, delim) == 0, self.last_error()
            pos, done, rc = 0, 0, 0
            while not (done and pos == len(z)):
                n = len(z) - pos if not feeds else min(feeds, len(z) - pos)
                buf = C.create_string_buffer(z[pos:pos + n], max(n, 1))
                used, d = C.c_size_t(0), C.c_int(0)
                rc = self.lib.bzx_index_feed(h, C.addressof(buf), n, int(pos + n == len(z)), C.byref(used), C.byref(d))
                if rc:
                    break
                assert used.value or d.value or n == 0
                pos += used.value
                done = d.value
            ep, info = C.POINTER(IndexEntry)(), IndexInfo()
            assert self.lib.bzx_index_get(h, C.byref(ep), C.byref(info)) == 0
            tp, tn = U64P(), C.c_uint64(12345)
            rrc = self.lib.bzx_index_get_records(h, C.byref(tp), C.byref(tn))
            table = None
            if rrc == 0:
                assert tn.value == info.nblk
                table = [tp[i] for i in range(tn.value + 1)]
            return rc, [ep[i].key() for i in range(info.nblk)], info, table if delim is not None else rrc
        finally:
            self.lib.bzx_index_end(h)

    def records_count_buffer(self, raw, delim, entries, n):
        table = u64([0xA5A5] * (n + 1))
        rc = self.lib.bzx_records_count_buffer(self.ctx, bytes(raw), len(raw), delim, entries, n, table)
        return rc, list(table[:n + 1])

    # ---- locate and read
    @staticmethod
    def _pieces(z, pieces):
        pieces = [(0, len(z))] if pieces is None else pieces
        bufs = [C.create_string_buffer(bytes(z[b:b + ln]), max(ln, 1)) for b, ln in pieces]
        return bufs, (Piece * max(len(pieces), 1))(*[Piece(C.addressof(bf), b, ln) for bf, (b, ln) in zip(bufs, pieces)]), len(pieces)

    def locate_raw(self, fn, pc, npc, entries, n, table, delim, recs):
        count = len(recs)
        offs, status = u64([77] * count), (C.c_int * max(count, 1))(*[77] * max(count, 1))
        rc = fn(self.ctx, pc, npc, entries, n, u64(table), delim, count, u64(recs), offs, status)
        return rc, list(offs[:count]), list(status[:count])

    def locate_buffer(self, z, pieces, entries, n, table, delim, recs):
        """bzx_records_locate_buffer; pieces: [(base, len)] of z (None: the whole file) -> (rc, byte_offs, status)."""
        bufs, pc, npc = self._pieces(z, pieces)
        return self.locate_raw(self.lib.bzx_records_locate_buffer, pc, npc, entries, n, table, delim, recs)

    def records_raw(self, fn, pc, npc, entries, n, table, delim, ranges, out, cap):
        count = len(ranges)
        offs, gots = (C.c_size_t * max(count, 1))(*[77] * max(count, 1)), (C.c_size_t * max(count, 1))(*[77] * max(count, 1))
        status, need = (C.c_int * max(count, 1))(*[77] * max(count, 1)), C.c_size_t(12345)
        rc = fn(self.ctx, pc, npc, entries, n, u64(table), delim, count, u64([r[0] for r in ranges]), u64([r[1] for r in ranges]),
                out, cap, offs, gots, status, C.byref(need))
        return RangesResult(rc, need.value, list(offs[:count]), list(gots[:count]), list(status[:count]), None)

    def records_buffer(self, z, pieces, entries, n, table, delim, ranges, cap, fill=0xA5):
        """bzx_decompress_records_buffer -> RangesResult (data(i): the bytes of range i)."""
        bufs, pc, npc = self._pieces(z, pieces)
        out = C.create_string_buffer(bytes([fill]) * max(cap, 1), max(cap, 1))
        r = self.records_raw(self.lib.bzx_decompress_records_buffer, pc, npc, entries, n, table, delim, ranges, C.addressof(out), cap)
        r.room = out.raw[:cap]
        return r

    # ---- the kernels alone
    def stage_count(self, buf, segs, delim):
        """segs: [(off, len)] -> (rc, [count])"""
        out = u32([0x5A5A5A5A] * len(segs))
        rc = self.lib.bzx_stage_rec_count(self.ctx, bytes(buf), len(buf), len(segs), u64([s[0] for s in segs]),
                                          u64([s[1] for s in segs]), delim, out)
        return rc, list(out[:len(segs)])

    def stage_select(self, buf, queries, delim):
        """queries: [(off, len, j)] -> (rc, [pos], [cnt])"""
        n = len(queries)
        pos, cnt = u32([0x5A5A5A5A] * n), u32([0x5A5A5A5A] * n)
        rc = self.lib.bzx_stage_rec_select(self.ctx, bytes(buf), len(buf), n, u64([q[0] for q in queries]),
                                           u64([q[1] for q in queries]), u32([q[2] for q in queries]), delim, pos, cnt)
        return rc, list(pos[:n]), list(cnt[:n])


__all__ = ["RecordsLib", "Planners", "planners", "pack_bzxr", "read_bzxr", "NONE", "IndexEntry", "IndexInfo", "u64"]
