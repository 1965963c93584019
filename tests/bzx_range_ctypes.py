"""ctypes bindings of the block index and the range reads (include/bzx.h: bzx_index_*, bzx_index_span,
bzx_decompress_range_*, bzx_stage_ibwt), used by the range tests, their probe and the command-line test.  RangeLib is
the DStreamLib of bzx_dstream_ctypes.py with those functions bound."""
import ctypes as C
import struct

from bzx_ctypes import BzxError, LIB_PATH
from bzx_dstream_ctypes import DStreamLib


class IndexEntry(C.Structure):
    _fields_ = [("bit", C.c_uint64), ("out_off", C.c_uint64), ("out_len", C.c_uint32), ("crc", C.c_uint32),
                ("img_bits", C.c_uint32), ("stream", C.c_uint32), ("level", C.c_uint8), ("reserved", C.c_uint8 * 7)]

    def key(self):
        return (self.bit, self.out_off, self.out_len, self.crc, self.img_bits, self.stream, self.level)


class IndexInfo(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("nblk", C.c_uint64), ("nstreams", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(IndexEntry) == 40 and C.sizeof(IndexInfo) == 32

BZXI_HEADER = struct.Struct("<4sIQQQI28x")       # magic, version, in_bytes, out_bytes, nblk, nstreams; 64 bytes


def read_bzxi(path):
    """A stored index -> (info fields as a dict, array of IndexEntry)."""
    with open(path, "rb") as f:
        raw = f.read()
    magic, version, in_bytes, out_bytes, nblk, nstreams = BZXI_HEADER.unpack_from(raw)
    assert magic == b"BZXI" and version == 1 and len(raw) == 64 + 40 * nblk
    entries = (IndexEntry * max(nblk, 1)).from_buffer_copy(raw[64:] + bytes(40 if nblk == 0 else 0))
    return {"in_bytes": in_bytes, "out_bytes": out_bytes, "nblk": nblk, "nstreams": nstreams}, entries


class RangeLib(DStreamLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        L = self.lib
        L.bzx_index_begin.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.bzx_index_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.bzx_index_get.argtypes = [C.c_void_p, C.POINTER(C.POINTER(IndexEntry)), C.POINTER(IndexInfo)]
        L.bzx_index_end.argtypes = [C.c_void_p]
        L.bzx_index_end.restype = None
        L.bzx_index_build_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_uint64, C.POINTER(IndexInfo)]
        L.bzx_index_span.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64] + [C.POINTER(C.c_uint64)] * 4
        for fn in (L.bzx_decompress_range_device, L.bzx_decompress_range_buffer):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                           C.c_void_p, C.POINTER(C.c_size_t)]
        L.bzx_stage_ibwt_time.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_float)]
        L.bzx_stage_ibwt.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]

    # ---- index
    def index_feed(self, z, feeds=0, max_chunk=0):
        """bzx_index_* over z cut into pieces of `feeds` bytes (0: everything at once) -> (rc, [entry keys], info, error text)."""
        h = C.c_void_p()
        rc = self.lib.bzx_index_begin(self.ctx, max_chunk, C.byref(h))
        if rc:
            raise BzxError(f"bzx_index_begin: {self.last_error()}", rc)
        try:
            pos, done, rc, calls = 0, 0, 0, 0
            while not (done and pos == len(z)):
                calls += 1
                assert calls < 10_000_000, "the feed loop does not end"
                n = len(z) - pos if not feeds else min(feeds, len(z) - pos)
                buf = C.create_string_buffer(z[pos:pos + n], max(n, 1))
                used, d = C.c_size_t(12345), C.c_int(12345)
                rc = self.lib.bzx_index_feed(h, C.addressof(buf), n, int(pos + n == len(z)), C.byref(used), C.byref(d))
                if rc:
                    break
                assert used.value <= n
                assert used.value or d.value or n == 0, "a feed call made no progress"
                pos += used.value
                done = d.value
            why = self.last_error()
            ep, info = C.POINTER(IndexEntry)(), IndexInfo()
            assert self.lib.bzx_index_get(h, C.byref(ep), C.byref(info)) == 0
            keys = [ep[i].key() for i in range(info.nblk)]
            return rc, keys, info, why
        finally:
            self.lib.bzx_index_end(h)

    def index_build(self, z, cap=None):
        """bzx_index_build_buffer -> (rc, array of IndexEntry (the first nblk are valid), info)."""
        if cap is None:
            cap = len(z) // 32 + 64
        entries = (IndexEntry * max(cap, 1))()
        info = IndexInfo()
        rc = self.lib.bzx_index_build_buffer(self.ctx, bytes(z), len(z), entries, cap, C.byref(info))
        return rc, entries, info

    def span(self, entries, n, off, want):
        v = [C.c_uint64() for _ in range(4)]
        rc = self.lib.bzx_index_span(entries, n, off, want, *[C.byref(x) for x in v])
        return (rc,) + tuple(x.value for x in v)                 # rc, first, count, byte_lo, byte_hi

    # ---- range reads
    def range_buffer(self, z, base, entries, n, off, want, room=None, fill=0xA5):
        """bzx_decompress_range_buffer with z = input bytes [base, base + len(z)) -> (rc, bytes delivered, the whole
        output buffer as left by the call)."""
        room = want if room is None else room
        out = C.create_string_buffer(bytes([fill]) * max(room, 1), max(room, 1))
        got = C.c_size_t(12345)
        buf = C.create_string_buffer(bytes(z), max(len(z), 1))
        rc = self.lib.bzx_decompress_range_buffer(self.ctx, C.addressof(buf), len(z), base, entries, n, off, want,
                                                  C.addressof(out), C.byref(got))
        return rc, out.raw[:got.value], out.raw[:room], got.value

    def range_device_raw(self, d_z, zlen, base, entries, n, off, want, d_out):
        got = C.c_size_t(12345)
        rc = self.lib.bzx_decompress_range_device(self.ctx, d_z, zlen, base, entries, n, off, want, d_out, C.byref(got))
        return rc, got.value

    # ---- the inverse BWT alone
    def stage_ibwt(self, L, orig_ptr, wide, raw_cap=None):
        """-> (img, raw, raw_len, status)"""
        n = len(L)
        raw_cap = (n // 5 * 259 + n % 5 + 16) if raw_cap is None else raw_cap
        img, raw = C.create_string_buffer(max(n, 1)), C.create_string_buffer(max(raw_cap, 1))
        rl, st = C.c_uint64(), C.c_uint32(12345)
        self._check(self.lib.bzx_stage_ibwt(self.ctx, bytes(L), n, orig_ptr, int(wide), img, raw, raw_cap, C.byref(rl),
                                            C.byref(st)))
        return img.raw[:n], (raw.raw[:min(rl.value, raw_cap)] if st.value == 0 else b""), rl.value, st.value


__all__ = ["RangeLib", "IndexEntry", "IndexInfo", "read_bzxi", "BzxError"]
