"""ctypes bindings of the batched decompression entry points (include/bzx.h: bzx_decompress_batch_*), used by the
batch decompression tests, its probe and the command-line test.  DBatchLib is the BatchLib of bzx_batch_ctypes.py with
the two decompression functions bound."""
import ctypes as C

from bzx_batch_ctypes import BatchLib
from bzx_ctypes import BzxError, LIB_PATH


class DBatchLib(BatchLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        L = self.lib
        for fn in (L.bzx_decompress_batch_device, L.bzx_decompress_batch_buffer):
            fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bzx_decompress_buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]
        L.bzx_decompress_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]

    def _call(self, fn, ptrs, lens, outs, caps, arrays=True):
        n = len(lens)
        m = max(n, 1)
        p = (C.c_void_p * m)(*ptrs) if arrays else None
        ln = (C.c_size_t * m)(*lens)
        o = (C.c_void_p * m)(*outs)
        cp = (C.c_size_t * m)(*caps)
        ol = (C.c_size_t * m)()
        st = (C.c_int * m)(*([12345] * m))
        rc = fn(self.ctx, n, p, ln, o, cp, ol, st)
        return rc, list(ol[:n]), list(st[:n])

    def dbatch_buffer_raw(self, ptrs, lens, outs, caps):
        """bzx_decompress_batch_buffer with host pointers (ints or None); returns (rc, out_lens, status)."""
        return self._call(self.lib.bzx_decompress_batch_buffer, ptrs, lens, outs, caps)

    def dbatch_device_raw(self, d_ptrs, lens, d_outs, caps):
        """bzx_decompress_batch_device with device pointers (ints or None); returns (rc, out_lens, status)."""
        return self._call(self.lib.bzx_decompress_batch_device, d_ptrs, lens, d_outs, caps)

    def dbatch_buffer(self, inputs, caps=None):
        """inputs: list of bytes -> (rc, [bytes or None], out_lens, status); caps default to 6 x input + 1 MiB."""
        bufs = [C.create_string_buffer(bytes(x), max(len(x), 1)) for x in inputs]
        lens = [len(x) for x in inputs]
        if caps is None:
            caps = [6 * n + (1 << 20) for n in lens]
        outs = [C.create_string_buffer(max(c, 1)) for c in caps]
        rc, olen, st = self.dbatch_buffer_raw([C.addressof(b) for b in bufs], lens, [C.addressof(o) for o in outs], caps)
        got = [C.string_at(C.addressof(o), n) if s == 0 else None for o, n, s in zip(outs, olen, st)]
        return rc, got, olen, st

    def decompress_one(self, z, cap=None):
        """bzx_decompress_buffer on one input -> (rc, bytes or None, out_len)."""
        if cap is None:
            cap = 6 * len(z) + (1 << 20)
        out = C.create_string_buffer(max(cap, 1))
        ol = C.c_size_t()
        rc = self.lib.bzx_decompress_buffer(self.ctx, bytes(z), len(z), out, cap, C.byref(ol))
        return rc, (out.raw[:ol.value] if rc == 0 else None), ol.value


__all__ = ["DBatchLib", "BzxError"]
