"""ctypes bindings of the streaming decompressor (include/bzx.h: bzx_dstream_*), used by the stream decompression
tests, its probe and the command-line test.  DStreamLib is the DBatchLib of bzx_dbatch_ctypes.py with the four stream
functions bound; dstream_decode drives the feed loop."""
import ctypes as C

from bzx_ctypes import BzxError, LIB_PATH
from bzx_dbatch_ctypes import DBatchLib


class DStreamInfo(C.Structure):
    _fields_ = [("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("nblk", C.c_uint32), ("nstreams", C.c_uint32),
                ("slabs", C.c_uint32), ("windows", C.c_uint32), ("rounds", C.c_uint32), ("scans", C.c_uint32),
                ("device_bytes", C.c_uint64), ("pinned_bytes", C.c_uint64)]


class DStream:
    """One open stream: feed(piece, final, cap) -> (rc, consumed, bytes produced, done)."""

    def __init__(self, lib, max_chunk=0):
        self.lib = lib
        self.h = C.c_void_p()
        rc = lib.lib.bzx_dstream_begin(lib.ctx, max_chunk, C.byref(self.h))
        if rc:
            raise BzxError(f"bzx_dstream_begin: {lib.last_error()}", rc)
        self._out = None

    def feed_raw(self, ptr, n, final, out_ptr, cap):
        """Pointers as ints (or None); returns (rc, consumed, produced, done)."""
        used, made, done = C.c_size_t(12345), C.c_size_t(12345), C.c_int(12345)
        rc = self.lib.lib.bzx_dstream_feed(self.h, ptr, n, int(final), C.byref(used), out_ptr, cap, C.byref(made),
                                           C.byref(done))
        return rc, used.value, made.value, done.value

    def feed(self, piece, final, cap):
        if self._out is None or len(self._out) < cap:
            self._out = C.create_string_buffer(max(cap, 1))
        buf = C.create_string_buffer(bytes(piece), max(len(piece), 1))
        rc, used, made, done = self.feed_raw(C.addressof(buf), len(piece), final, C.addressof(self._out), cap)
        return rc, used, C.string_at(C.addressof(self._out), made) if rc == 0 else b"", done

    def info(self):
        i = DStreamInfo()
        rc = self.lib.lib.bzx_dstream_get_info(self.h, C.byref(i))
        if rc:
            raise BzxError("bzx_dstream_get_info", rc)
        return i

    def end(self):
        if self.h:
            self.lib.lib.bzx_dstream_end(self.h)
            self.h = C.c_void_p()


class DStreamLib(DBatchLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        L = self.lib
        L.bzx_dstream_begin.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.bzx_dstream_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.c_void_p,
                                       C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.bzx_dstream_end.argtypes = [C.c_void_p]
        L.bzx_dstream_end.restype = None
        L.bzx_dstream_get_info.argtypes = [C.c_void_p, C.POINTER(DStreamInfo)]

    def dstream(self, max_chunk=0):
        return DStream(self, max_chunk)


def _cycle(v):
    """An int, a sequence (cycled) or a callable -> a callable giving the next size."""
    if callable(v):
        return v
    if isinstance(v, int):
        return lambda: v
    seq = list(v)
    state = {"i": 0}

    def nxt():
        x = seq[state["i"] % len(seq)]
        state["i"] += 1
        return x
    return nxt


def dstream_decode(lib, z, feeds, caps, max_chunk=0, sink=None, limit=10_000_000):
    """Drives the feed loop over z.  feeds / caps: piece sizes and cap values (int, cycled sequence or callable;
    a feed size of 0 or None = everything left).  Returns (rc, bytes, info): rc is the final status, bytes everything
    delivered (to sink(piece) instead when given), info the stream's figures before bzx_dstream_end.  Checks the loop
    contract on the way: consumed <= len, produced <= cap, progress in every call."""
    nf, nc = _cycle(feeds), _cycle(caps)
    s = lib.dstream(max_chunk)
    out = []
    try:
        info0 = s.info()
        pos, rc, done, calls = 0, 0, 0, 0
        while not done:
            calls += 1
            assert calls < limit, "the feed loop does not end"
            want = nf()
            n = len(z) - pos if not want else min(want, len(z) - pos)
            final = pos + n == len(z)
            cap = nc()
            rc, used, got, done = s.feed(z[pos:pos + n], final, cap)
            if rc:
                break
            assert used <= n and len(got) <= cap
            assert used or got or done or cap == 0 or (n == 0 and not final), "a call with room made no progress"
            pos += used
            if sink:
                sink(got)
            else:
                out.append(got)
        info = s.info()
        assert info.device_bytes == info0.device_bytes and info.pinned_bytes == info0.pinned_bytes
        assert info.slabs == info0.slabs
        if rc:                                        # sticky
            rc2, used, got, done = s.feed(b"", True, 16)
            assert rc2 == rc and not used and not got and not done
        return rc, b"".join(out), info
    finally:
        s.end()


__all__ = ["DStreamLib", "DStream", "DStreamInfo", "dstream_decode", "BzxError"]
