"""ctypes bindings of the index the compressor keeps (include/bzx.h: bzx_ctx_keep_index, bzx_compress_get_index,
bzx_cstream_get_index, bzx_compress_batch_get_index and the bzx_mctx / bzx_mstream forms), used by the compress-index
tests, their probe and the command-line test.  CIndexLib is a RangeLib with the batch calls and those functions bound;
the m_* functions work on an MDev of bzx_mdev_ctypes.py.  Entries travel as their 40 stored bytes, so that a comparison
is a memcmp."""
import ctypes as C
import struct

from bzx_batch_ctypes import BatchLib
from bzx_ctypes import BzxError, LIB_PATH
from bzx_range_ctypes import IndexEntry, IndexInfo, RangeLib

ENTRY = struct.Struct("<QQIIIIB7x")              # bit, out_off, out_len, crc, img_bits, stream, level, reserved
assert ENTRY.size == 40

_GET = [C.c_void_p, C.POINTER(C.POINTER(IndexEntry)), C.POINTER(IndexInfo)]


def info_tuple(info):
    return (info.in_bytes, info.out_bytes, info.nblk, info.nstreams, info.reserved)


def _get(fn, handle):
    """-> (rc, the entries as bytes, (in_bytes, out_bytes, nblk, nstreams, reserved))"""
    ep, info = C.POINTER(IndexEntry)(), IndexInfo()
    rc = fn(handle, C.byref(ep), C.byref(info))
    if rc:
        return rc, b"", None
    return 0, (C.string_at(ep, 40 * info.nblk) if info.nblk else b""), info_tuple(info)


def bind(L):
    L.bzx_ctx_keep_index.argtypes = [C.c_void_p, C.c_int]
    L.bzx_mctx_keep_index.argtypes = [C.c_void_p, C.c_int]
    for fn in (L.bzx_compress_get_index, L.bzx_cstream_get_index, L.bzx_mctx_get_index, L.bzx_mstream_get_index):
        fn.argtypes = _GET
    L.bzx_compress_batch_get_index.argtypes = [C.c_void_p, C.POINTER(C.POINTER(IndexEntry)),
                                               C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint32)]
    return L


class CIndexLib(RangeLib, BatchLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        bind(self.lib)

    def keep_index(self, on):
        return self.lib.bzx_ctx_keep_index(self.ctx, int(on))

    def compress_get_index(self):
        return _get(self.lib.bzx_compress_get_index, self.ctx)

    def cstream_get_index(self, stream):
        return _get(self.lib.bzx_cstream_get_index, stream.h)

    def compress_buffer_rc(self, data, level, cap):
        out = C.create_string_buffer(max(cap, 1))
        ol = C.c_size_t(0)
        rc = self.lib.bzx_compress_buffer(self.ctx, bytes(data), len(data), level, out, cap, C.byref(ol))
        return rc, (out.raw[:ol.value] if rc == 0 else b"")

    def batch_get_index(self):
        """-> (rc, [the entries of stream i as bytes])"""
        ep, fp, n = C.POINTER(IndexEntry)(), C.POINTER(C.c_uint64)(), C.c_uint32(12345)
        rc = self.lib.bzx_compress_batch_get_index(self.ctx, C.byref(ep), C.byref(fp), C.byref(n))
        if rc:
            return rc, []
        first = [fp[i] for i in range(n.value + 1)]
        assert first[0] == 0 and first == sorted(first)
        raw = C.string_at(ep, 40 * first[-1]) if first[-1] else b""
        return 0, [raw[40 * first[i]:40 * first[i + 1]] for i in range(n.value)]

    def index_build_bytes(self, z):
        """bzx_index_build_buffer -> (the entries as bytes, info tuple)."""
        rc, entries, info = self.index_build(z)
        if rc:
            raise BzxError(f"bzx_index_build_buffer: {rc}: {self.last_error()}", rc)
        return C.string_at(entries, 40 * info.nblk) if info.nblk else b"", info_tuple(info)


def m_keep_index(md, on):
    return bind(md.lib).bzx_mctx_keep_index(md.h, int(on))


def m_get_index(md):
    return _get(bind(md.lib).bzx_mctx_get_index, md.h)


def ms_get_index(md, stream):
    return _get(bind(md.lib).bzx_mstream_get_index, stream.h)


def entries_from_bytes(raw):
    """Stored entries -> a ctypes array for the range reads (one spare element when there is none)."""
    n = len(raw) // 40
    return (IndexEntry * max(n, 1)).from_buffer_copy(raw + bytes(40 if n == 0 else 0)), n


__all__ = ["CIndexLib", "ENTRY", "bind", "info_tuple", "m_keep_index", "m_get_index", "ms_get_index",
           "entries_from_bytes", "BzxError"]
