"""ctypes bindings of the find layer (include/bzx.h: bzx_index_find, bzx_index_get_hits, bzx_find_buffer,
bzx_find_geometry, bzx_stage_find), used by the find tests, the command-line test and the probe.  FindLib is the
RecordsLib of bzx_records_ctypes.py with those functions bound."""
import ctypes as C

from bzx_ctypes import LIB_PATH
from bzx_range_ctypes import IndexEntry, IndexInfo
from bzx_records_ctypes import RecordsLib, u32, u64

U64P, U32P = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


def geometry(path=LIB_PATH):
    """bzx_find_geometry: no context, no device -> (tile_bytes, inline_hits, window_hits)"""
    lib = C.CDLL(path)
    lib.bzx_find_geometry.restype = None
    v = [C.c_uint32(0) for _ in range(3)]
    lib.bzx_find_geometry(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


class FindLib(RecordsLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        RecordsLib.__init__(self, path, device, max_blocks)
        L = self.lib
        L.bzx_index_find.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64]
        L.bzx_index_get_hits.argtypes = [C.c_void_p, C.POINTER(U64P), U64P, U64P]
        L.bzx_find_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, U64P, C.c_uint64, U64P, U64P,
                                      C.c_void_p, C.c_uint64, C.POINTER(IndexInfo)]
        L.bzx_stage_find.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, U64P, U64P, C.c_char_p, C.c_size_t,
                                     C.c_uint64, C.c_uint32, U32P, U64P, U32P]

    def find_buffer(self, z, pat, cap_hits, cap_entries=None, want_entries=True):
        """bzx_find_buffer -> (rc, [hits listed], total, entries, info)"""
        cap_entries = (len(z) // 32 + 64 if cap_entries is None else cap_entries) if want_entries else 0
        entries = (IndexEntry * max(cap_entries, 1))() if want_entries else None
        hits, info = (C.c_uint64 * max(cap_hits, 1))(), IndexInfo()
        nl, total = C.c_uint64(12345), C.c_uint64(12345)
        rc = self.lib.bzx_find_buffer(self.ctx, bytes(z), len(z), bytes(pat), len(pat), hits, cap_hits, C.byref(nl),
                                      C.byref(total), entries, cap_entries, C.byref(info))
        assert nl.value <= cap_hits
        return rc, list(hits[:nl.value]), total.value, entries, info

    def get_hits(self, h):
        """bzx_index_get_hits -> (rc, [hits listed], total)"""
        hp, nl, total = U64P(), C.c_uint64(12345), C.c_uint64(12345)
        rc = self.lib.bzx_index_get_hits(h, C.byref(hp), C.byref(nl), C.byref(total))
        return rc, ([hp[i] for i in range(nl.value)] if rc == 0 else None), (total.value if rc == 0 else None)

    def index_feed_find(self, z, pat, max_hits, feeds=0, max_chunk=0, delim=None, watch=False):
        """bzx_index_* with find (pat None: off) over z in pieces of `feeds` bytes
        -> (rc, [entry keys], info, hits rc, [hits], total, record table or None, [hit lists seen between the feeds])"""
        h = C.c_void_p()
        assert self.lib.bzx_index_begin(self.ctx, max_chunk, C.byref(h)) == 0, self.last_error()
        try:
            if delim is not None:
                assert self.lib.bzx_index_count_records(h, delim) == 0, self.last_error()
            if pat is not None:
                assert self.lib.bzx_index_find(h, bytes(pat), len(pat), max_hits) == 0, self.last_error()
            pos, done, rc, seen = 0, 0, 0, []
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
                if watch:
                    seen.append(self.get_hits(h)[1])
            why = self.last_error()
            ep, info = C.POINTER(IndexEntry)(), IndexInfo()
            assert self.lib.bzx_index_get(h, C.byref(ep), C.byref(info)) == 0
            keys = [ep[i].key() for i in range(info.nblk)]
            hrc, hits, total = self.get_hits(h)
            table = None
            if delim is not None:
                tp, tn = U64P(), C.c_uint64(12345)
                assert self.lib.bzx_index_get_records(h, C.byref(tp), C.byref(tn)) == 0 and tn.value == info.nblk
                table = [tp[i] for i in range(tn.value + 1)]
            self.why = why
            return rc, keys, info, hrc, hits, total, table, seen
        finally:
            self.lib.bzx_index_end(h)

    def stage_find(self, buf, segs, pat, skip=0, cap=0):
        """segs: [(off, len)] -> (rc, [count], [hits written])"""
        counts, out, nw = u32([0x5A5A5A5A] * len(segs)), (C.c_uint64 * max(cap, 1))(), C.c_uint32(12345)
        rc = self.lib.bzx_stage_find(self.ctx, bytes(buf), len(buf), len(segs), u64([s[0] for s in segs]),
                                     u64([s[1] for s in segs]), bytes(pat) if pat is not None else None,
                                     len(pat) if pat is not None else 0, skip, cap, counts, out, C.byref(nw))
        if rc:
            return rc, None, None
        assert nw.value <= cap
        return rc, list(counts[:len(segs)]), list(out[:nw.value])


__all__ = ["FindLib", "geometry", "IndexEntry", "IndexInfo", "u64"]
