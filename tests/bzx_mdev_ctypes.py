"""ctypes bindings of the single-process multi-device compressor (include/bzx.h: bzx_mctx_*, bzx_mstream_*,
bzx_mcompress_buffer, bzx_stage_shift_bits), used by the multi-device tests, their probe and the command-line test."""
import ctypes as C
import os

from bzx_ctypes import BzxError, BzxStats, LIB_PATH

BZX_MAX_DEVICES = 64
E_NODEVICE, E_PARAM, E_NOMEM, E_OUTBUF, E_HIP, E_STATE = -1, -2, -3, -4, -5, -6


class MDevEntry(C.Structure):
    _fields_ = [("device", C.c_int32), ("chunks", C.c_uint32), ("blocks", C.c_uint64), ("ms_device", C.c_float),
                ("reserved", C.c_uint32), ("device_bytes", C.c_uint64), ("pinned_bytes", C.c_uint64)]


class MDevInfo(C.Structure):
    _fields_ = [("ndev", C.c_uint32), ("chunks", C.c_uint32), ("shifted", C.c_uint32), ("reserved", C.c_uint32),
                ("nblk", C.c_uint64), ("dev", MDevEntry * BZX_MAX_DEVICES)]


def bind(L):
    L.bzx_mctx_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.bzx_mctx_destroy.argtypes = [C.c_void_p]
    L.bzx_mctx_destroy.restype = None
    L.bzx_mctx_last_error.argtypes = [C.c_void_p]
    L.bzx_mctx_last_error.restype = C.c_char_p
    L.bzx_mcompress_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]
    L.bzx_mstream_begin.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.bzx_mstream_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    L.bzx_mstream_end.argtypes = [C.c_void_p]
    L.bzx_mstream_end.restype = None
    L.bzx_mctx_get_stats.argtypes = [C.c_void_p, C.POINTER(BzxStats)]
    L.bzx_mctx_get_info.argtypes = [C.c_void_p, C.POINTER(MDevInfo)]
    L.bzx_stage_shift_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.bzx_host_alloc.argtypes = [C.c_size_t]
    L.bzx_host_alloc.restype = C.c_void_p
    L.bzx_host_free.argtypes = [C.c_void_p]
    L.bzx_host_free.restype = None
    return L


def mctx_create_rc(L, devices, ndev=None, max_blocks=16, null_list=False, null_out=False):
    """The return code of bzx_mctx_create alone (a created object is destroyed again)."""
    n = len(devices) if ndev is None else ndev
    arr = (C.c_int * max(len(devices), 1))(*devices)
    h = C.c_void_p()
    rc = L.bzx_mctx_create(None if null_list else arr, n, max_blocks, None if null_out else C.byref(h))
    if h:
        L.bzx_mctx_destroy(h)
    return rc


class MStream:
    """One open stream: feed_raw(ptr, n, final, out_ptr, cap) -> (rc, produced)."""

    def __init__(self, md, level, max_chunk):
        self.md = md
        self.h = C.c_void_p()
        rc = md.lib.bzx_mstream_begin(md.h, level, max_chunk, C.byref(self.h))
        if rc:
            raise BzxError(f"bzx_mstream_begin: {md.last_error()}", rc)

    def feed_raw(self, ptr, n, final, out_ptr, cap):
        made = C.c_size_t(0)
        rc = self.md.lib.bzx_mstream_feed(self.h, ptr, n, int(final), out_ptr, cap, C.byref(made))
        return rc, made.value

    def end(self):
        if self.h:
            self.md.lib.bzx_mstream_end(self.h)
            self.h = C.c_void_p()


class MDev:
    """A bzx_mctx over `devices` (a sequence of HIP ordinals, repeats allowed)."""

    def __init__(self, devices, path=LIB_PATH, max_blocks=16):
        if not os.path.exists(path):
            raise BzxError(f"{path} missing: build it with __graft_entry__.build() (no CPU fallback exists)")
        self.lib = bind(C.CDLL(path))
        self.devices = tuple(devices)
        self.h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        rc = self.lib.bzx_mctx_create(arr, len(devices), max_blocks, C.byref(self.h))
        if rc:
            raise BzxError(f"bzx_mctx_create{self.devices}: {rc}", rc)

    def last_error(self):
        return self.lib.bzx_mctx_last_error(self.h).decode()

    def close(self):
        if self.h:
            self.lib.bzx_mctx_destroy(self.h)
            self.h = C.c_void_p()

    def stats(self):
        st = BzxStats()
        assert self.lib.bzx_mctx_get_stats(self.h, C.byref(st)) == 0
        return st

    def info(self):
        i = MDevInfo()
        assert self.lib.bzx_mctx_get_info(self.h, C.byref(i)) == 0
        return i

    def compress_buffer_rc(self, data, level, cap):
        """bzx_mcompress_buffer with a given cap -> (rc, bytes, *out_len)."""
        out = C.create_string_buffer(max(cap, 1))
        src = C.create_string_buffer(bytes(data), max(len(data), 1))
        ol = C.c_size_t(0)
        rc = self.lib.bzx_mcompress_buffer(self.h, C.addressof(src), len(data), level, C.addressof(out), cap, C.byref(ol))
        return rc, (out.raw[:ol.value] if rc == 0 else b""), ol.value

    def compress_buffer(self, data, level=9):
        rc, z, _ = self.compress_buffer_rc(data, level, len(data) + len(data) // 50 + 4096)
        if rc:
            raise BzxError(f"bzx_mcompress_buffer: {rc}: {self.last_error()}", rc)
        return z

    def compress_ptr(self, src_ptr, n, level, out_ptr, cap):
        """Raw pointers (page-locked buffers of the probes and GPU tests) -> stream length."""
        ol = C.c_size_t(0)
        rc = self.lib.bzx_mcompress_buffer(self.h, src_ptr, n, level, out_ptr, cap, C.byref(ol))
        if rc:
            raise BzxError(f"bzx_mcompress_buffer: {rc}: {self.last_error()}", rc)
        return ol.value

    def mstream(self, level=9, max_chunk=0):
        return MStream(self, level, max_chunk)

    def mstream_compress(self, data, level=9, chunk=1 << 20, max_chunk=None, empty_final=False, pinned=False,
                         after_feed=None):
        """bzx_mstream_*: feed `data` in pieces of `chunk` bytes (an int, or a list of piece lengths, cycled); with
        empty_final the last bytes go in a call without `final` and a call with len == 0 completes the stream.
        pinned: source and destination in bzx_host_alloc memory.  after_feed(k): called after the k-th feed.
        Checks on the way that *produced never shrinks and that the last 64 bytes it covered (the neighbourhood of the
        word two chunks share) have not changed by the next call; the caller compares the whole stream."""
        pieces = list(chunk) if isinstance(chunk, (list, tuple)) else None
        mc = max_chunk or (max(pieces) if pieces else chunk)
        cap = len(data) + len(data) // 50 + 4096
        L = self.lib
        if pinned:
            p_src, p_out = L.bzx_host_alloc(max(len(data), 1)), L.bzx_host_alloc(cap)
            assert p_src and p_out
            C.memmove(p_src, bytes(data), len(data))
        else:
            src = C.create_string_buffer(bytes(data), max(len(data), 1))
            out = C.create_string_buffer(cap)
            p_src, p_out = C.addressof(src), C.addressof(out)
        s = self.mstream(level, mc)
        try:
            def edge(upto):
                return C.string_at(p_out + max(0, upto - 64), min(64, upto))

            off, i, last, prefix = 0, 0, 0, b""
            while True:
                n = min(len(data) - off, pieces[i % len(pieces)] if pieces else chunk)
                last_bytes = off + n >= len(data)
                fin = last_bytes and not empty_final
                rc, made = s.feed_raw(p_src + off, n, fin, p_out, cap)
                if rc:
                    raise BzxError(f"bzx_mstream_feed: {rc}: {self.last_error()}", rc)
                assert made >= last and edge(last) == prefix, "a byte reported final has changed"
                last, prefix = made, edge(made)
                if after_feed:
                    after_feed(i)
                off += n
                i += 1
                if fin:
                    break
                if last_bytes:
                    rc, made = s.feed_raw(None, 0, True, p_out, cap)
                    if rc:
                        raise BzxError(f"bzx_mstream_feed: {rc}: {self.last_error()}", rc)
                    assert made >= last and edge(last) == prefix
                    last = made
                    if after_feed:
                        after_feed(i)
                    break
            return C.string_at(p_out, last)
        finally:
            s.end()
            if pinned:
                L.bzx_host_free(p_src)
                L.bzx_host_free(p_out)


def shift_bits(bzxlib, data, p):
    """bzx_stage_shift_bits on a BzxLib's context -> the (len(data) + 4 rounded up to 4) output bytes."""
    L = bind(bzxlib.lib)
    n = len(data)
    outn = (n + 4 + 3) // 4 * 4
    out = C.create_string_buffer(b"\xa5" * outn, outn)
    src = C.create_string_buffer(bytes(data), max(n, 1))
    rc = L.bzx_stage_shift_bits(bzxlib.ctx, C.addressof(src), n, p, C.addressof(out))
    if rc:
        raise BzxError(f"bzx_stage_shift_bits: {rc}", rc)
    return out.raw[:outn]


def shift_bits_ref(data, p):
    """The same shift with Python's big integers."""
    n = len(data)
    outn = (n + 4 + 3) // 4 * 4
    return ((int.from_bytes(data, "big") << (8 * (outn - n))) >> p).to_bytes(outn, "big") if outn else b""


__all__ = ["MDev", "MStream", "MDevInfo", "BzxError", "bind", "mctx_create_rc", "shift_bits", "shift_bits_ref",
           "E_NODEVICE", "E_PARAM", "E_OUTBUF", "E_STATE", "BZX_MAX_DEVICES"]
