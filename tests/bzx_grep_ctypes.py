"""ctypes bindings of the grep layer (include/bzx.h: bzx_index_find_lines, bzx_index_get_hit_lines, bzx_grep_buffer,
bzx_stage_find_lines), used by the grep tests and the probe.  GrepLib is the FindLib of bzx_find_ctypes.py with those
functions bound."""
import ctypes as C

from bzx_ctypes import LIB_PATH
from bzx_find_ctypes import FindLib, IndexEntry, IndexInfo, U32P, U64P, geometry
from bzx_records_ctypes import u32, u64

SZP = C.POINTER(C.c_size_t)


class GrepLib(FindLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        FindLib.__init__(self, path, device, max_blocks)
        L = self.lib
        L.bzx_index_find_lines.argtypes = [C.c_void_p, C.c_int]
        L.bzx_index_get_hit_lines.argtypes = [C.c_void_p, C.POINTER(U64P), U64P]
        L.bzx_grep_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.c_uint64, U64P,
                                      C.c_uint64, U64P, C.c_char_p, C.c_size_t, SZP, SZP, SZP, U64P, C.POINTER(C.c_int)]
        L.bzx_stage_find_lines.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, U64P, U64P, C.c_char_p, C.c_size_t,
                                           C.c_int, C.c_uint64, C.c_uint32, U32P, U32P, U64P, U64P, U32P]

    def stage_find_lines(self, buf, segs, pat, delim, skip=0, cap=0):
        """segs: [(off, len)] -> (rc, [count], [delimiter count], [hits written], [their lines])"""
        n = len(segs)
        counts, dcounts = u32([0x5A5A5A5A] * n), u32([0x5A5A5A5A] * n)
        out, lout, nw = (C.c_uint64 * max(cap, 1))(), (C.c_uint64 * max(cap, 1))(), C.c_uint32(12345)
        rc = self.lib.bzx_stage_find_lines(self.ctx, bytes(buf), len(buf), n, u64([s[0] for s in segs]),
                                           u64([s[1] for s in segs]), bytes(pat) if pat is not None else None,
                                           len(pat) if pat is not None else 0, delim, skip, cap, counts, dcounts, out, lout,
                                           C.byref(nw))
        if rc:
            return rc, None, None, None, None
        assert nw.value <= cap
        return rc, list(counts[:n]), list(dcounts[:n]), list(out[:nw.value]), list(lout[:nw.value])

    def get_hit_lines(self, h):
        """bzx_index_get_hit_lines -> (rc, [lines] or None)"""
        lp, nl = U64P(), C.c_uint64(12345)
        rc = self.lib.bzx_index_get_hit_lines(h, C.byref(lp), C.byref(nl))
        return rc, ([lp[i] for i in range(nl.value)] if rc == 0 else None)

    def index_feed_lines(self, z, pat, max_hits, delim, feeds=0, max_chunk=0, rec_delim=None, lines=True):
        """bzx_index_* with find, lines (lines=False: find alone) and the record table (rec_delim None: off) over z in
        pieces of `feeds` bytes -> (rc, [entry keys], info, [hits], total, lines rc, [lines], record table or None)"""
        h = C.c_void_p()
        assert self.lib.bzx_index_begin(self.ctx, max_chunk, C.byref(h)) == 0, self.last_error()
        try:
            assert self.lib.bzx_index_find(h, bytes(pat), len(pat), max_hits) == 0, self.last_error()
            if lines:
                assert self.lib.bzx_index_find_lines(h, delim) == 0, self.last_error()
            if rec_delim is not None:
                assert self.lib.bzx_index_count_records(h, rec_delim) == 0, self.last_error()
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
            self.why = self.last_error()
            ep, info = C.POINTER(IndexEntry)(), IndexInfo()
            assert self.lib.bzx_index_get(h, C.byref(ep), C.byref(info)) == 0
            keys = [ep[i].key() for i in range(info.nblk)]
            hrc, hits, total = self.get_hits(h)
            assert hrc == 0
            lrc, lns = self.get_hit_lines(h)
            self.lines_why = self.last_error()
            table = None
            if rec_delim is not None:
                tp, tn = U64P(), C.c_uint64(12345)
                assert self.lib.bzx_index_get_records(h, C.byref(tp), C.byref(tn)) == 0 and tn.value == info.nblk
                table = [tp[i] for i in range(tn.value + 1)]
            return rc, keys, info, hits, total, lrc, lns, table
        finally:
            self.lib.bzx_index_end(h)

    def grep_buffer(self, z, pat, delim, max_hits, cap_recs, cap):
        """bzx_grep_buffer -> (rc, [recs], [record bytes], nrecs, need, total_hits, truncated); the lists hold what was
        written (nothing after an error other than BZX_E_DATA)"""
        recs = (C.c_uint64 * max(cap_recs, 1))()
        offs, lens = (C.c_size_t * max(cap_recs, 1))(), (C.c_size_t * max(cap_recs, 1))()
        out = C.create_string_buffer(max(cap, 1))
        nrecs, need, total, trunc = C.c_uint64(12345), C.c_size_t(12345), C.c_uint64(12345), C.c_int(12345)
        rc = self.lib.bzx_grep_buffer(self.ctx, bytes(z), len(z), bytes(pat), len(pat), delim, max_hits, recs, cap_recs,
                                      C.byref(nrecs), out, cap, offs, lens, C.byref(need), C.byref(total), C.byref(trunc))
        got_recs, got = [], []
        if rc in (0, -7):
            assert nrecs.value <= cap_recs and need.value <= cap
            got_recs = list(recs[:nrecs.value])
            at = 0
            for i in range(nrecs.value):                    # (packed, in list order)
                assert offs[i] == at
                got.append(out.raw[offs[i]:offs[i] + lens[i]])
                at += lens[i]
            assert at == need.value
        return rc, got_recs, got, nrecs.value, need.value, total.value, trunc.value


__all__ = ["GrepLib", "geometry", "IndexEntry", "IndexInfo"]
