"""ctypes bindings of the salvage calls (include/bzx.h: bzx_salvage_*, bzx_index_get_gaps), used by the salvage tests, their
probe and the command-line test.  SalvageLib is the RangeLib of bzx_range_ctypes.py with those functions bound."""
import ctypes as C

from bzx_ctypes import BzxError, LIB_PATH
from bzx_range_ctypes import IndexEntry, IndexInfo, RangeLib

GAP_STRUCTURE, GAP_BLOCK_CRC, GAP_RANDOMISED, GAP_NO_MAGIC, GAP_TRUNCATED, GAP_COMBINED_CRC, GAP_HEADER = 1, 2, 4, 8, 16, 32, 64


class Gap(C.Structure):
    _fields_ = [("bit_lo", C.c_uint64), ("bit_hi", C.c_uint64), ("out_off", C.c_uint64), ("candidates", C.c_uint32),
                ("why", C.c_uint32)]

    def key(self):
        return (self.bit_lo, self.bit_hi, self.out_off, self.candidates, self.why)


assert C.sizeof(Gap) == 32


class SalvageLib(RangeLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        L = self.lib
        L.bzx_salvage_begin.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.bzx_index_get_gaps.argtypes = [C.c_void_p, C.POINTER(C.POINTER(Gap)), C.POINTER(C.c_uint64)]
        L.bzx_salvage_build_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_uint64, C.POINTER(IndexInfo),
                                               C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.bzx_salvage_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]

    def salvage_feed(self, z, feeds=0, max_chunk=0):
        """bzx_salvage_begin and bzx_index_feed over z cut into pieces of `feeds` bytes (0: everything at once)
        -> (rc, [entry keys], info, [gap keys]).  *done may become 1 only with the final feed."""
        h = C.c_void_p()
        rc = self.lib.bzx_salvage_begin(self.ctx, max_chunk, C.byref(h))
        if rc:
            raise BzxError(f"bzx_salvage_begin: {self.last_error()}", rc)
        try:
            pos, done, rc, calls = 0, 0, 0, 0
            while not (done and pos == len(z)):
                calls += 1
                assert calls < 10_000_000, "the feed loop does not end"
                n = len(z) - pos if not feeds else min(feeds, len(z) - pos)
                final = int(pos + n == len(z))
                buf = C.create_string_buffer(z[pos:pos + n], max(n, 1))
                used, d = C.c_size_t(12345), C.c_int(12345)
                rc = self.lib.bzx_index_feed(h, C.addressof(buf), n, final, C.byref(used), C.byref(d))
                if rc:
                    break
                assert used.value <= n
                assert used.value or d.value or n == 0, "a feed call made no progress"
                assert not d.value or final, "done before the final feed"
                pos += used.value
                done = d.value
            ep, info = C.POINTER(IndexEntry)(), IndexInfo()
            assert self.lib.bzx_index_get(h, C.byref(ep), C.byref(info)) == 0
            gp, ng = C.POINTER(Gap)(), C.c_uint64()
            assert self.lib.bzx_index_get_gaps(h, C.byref(gp), C.byref(ng)) == 0
            return rc, [ep[i].key() for i in range(info.nblk)], info, [gp[i].key() for i in range(ng.value)]
        finally:
            self.lib.bzx_index_end(h)

    def salvage_build(self, z, cap=None, cap_gaps=None):
        """bzx_salvage_build_buffer -> (rc, array of IndexEntry (the first min(nblk, cap) are valid), info, [gap keys
        written], gaps needed)."""
        if cap is None:
            cap = len(z) // 32 + 64
        if cap_gaps is None:
            cap_gaps = len(z) // 32 + 64
        entries = (IndexEntry * max(cap, 1))()
        gaps = (Gap * max(cap_gaps, 1))()
        info, ng = IndexInfo(), C.c_uint64(12345)
        rc = self.lib.bzx_salvage_build_buffer(self.ctx, bytes(z), len(z), entries, cap, C.byref(info), gaps, cap_gaps,
                                               C.byref(ng))
        return rc, entries, info, [gaps[i].key() for i in range(min(ng.value, cap_gaps))], ng.value

    def salvage_buffer(self, z, cap, cap_gaps=64, fill=0xA5):
        """bzx_salvage_buffer -> (rc, the first min(out_len, cap) bytes of the output buffer, out_len, [gap keys written],
        gaps needed)."""
        out = C.create_string_buffer(bytes([fill]) * max(cap, 1), max(cap, 1))
        gaps = (Gap * max(cap_gaps, 1))()
        n, ng = C.c_size_t(12345), C.c_uint64(12345)
        rc = self.lib.bzx_salvage_buffer(self.ctx, bytes(z), len(z), out, cap, C.byref(n), gaps, cap_gaps, C.byref(ng))
        return rc, out.raw[:min(n.value, cap)], n.value, [gaps[i].key() for i in range(min(ng.value, cap_gaps))], ng.value


__all__ = ["SalvageLib", "Gap", "IndexEntry", "IndexInfo", "BzxError", "GAP_STRUCTURE", "GAP_BLOCK_CRC", "GAP_RANDOMISED",
           "GAP_NO_MAGIC", "GAP_TRUNCATED", "GAP_COMBINED_CRC", "GAP_HEADER"]
