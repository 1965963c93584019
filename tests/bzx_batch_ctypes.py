"""ctypes bindings of the batched compression entry points (include/bzx.h: bzx_compress_batch_*), used by the batch
tests, the batch probe and the command-line test.  BatchLib is a BzxLib with the three batch functions bound."""
import ctypes as C

from bzx_ctypes import BzxError, BzxLib, LIB_PATH


class BatchLib(BzxLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        L = self.lib
        L.bzx_compress_batch_bound.restype = C.c_size_t
        L.bzx_compress_batch_bound.argtypes = [C.c_uint32, C.c_void_p]
        L.bzx_compress_batch_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p]
        L.bzx_compress_batch_buffer.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_size_t, C.c_void_p, C.c_void_p]
        L.bzx_get_block_info.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]

    def last_error(self):
        return self.lib.bzx_last_error(self.ctx).decode()

    def batch_bound(self, lens):
        arr = (C.c_size_t * max(len(lens), 1))(*lens)
        return self.lib.bzx_compress_batch_bound(len(lens), arr)

    def batch_buffer_raw(self, ptrs, lens, level, out, cap):
        """bzx_compress_batch_buffer with host pointers ptrs (ints or None); returns (rc, offs, lens)."""
        n = len(lens)
        p = (C.c_void_p * max(n, 1))(*ptrs)
        ln = (C.c_size_t * max(n, 1))(*lens)
        offs = (C.c_size_t * max(n, 1))()
        olen = (C.c_size_t * max(n, 1))()
        rc = self.lib.bzx_compress_batch_buffer(self.ctx, n, p, ln, level, out, cap, offs, olen)
        return rc, list(offs[:n]), list(olen[:n])

    def batch_buffer(self, inputs, level=9, cap=None, whole=False):
        """inputs: list of bytes -> list of streams (whole=True: also the output buffer, offsets and lengths)."""
        bufs = [C.create_string_buffer(bytes(x), max(len(x), 1)) for x in inputs]
        lens = [len(x) for x in inputs]
        if cap is None:
            cap = self.batch_bound(lens)
        out = C.create_string_buffer(max(cap, 1))
        rc, offs, olen = self.batch_buffer_raw([C.addressof(b) for b in bufs], lens, level, out, cap)
        self._check(rc)
        raw = out.raw                              # (one copy: .raw copies the whole buffer on every access)
        streams = [raw[o:o + n] for o, n in zip(offs, olen)]
        return (streams, raw, offs, olen) if whole else streams

    def batch_device_raw(self, d_ptrs, lens, level, d_out, cap):
        """bzx_compress_batch_device with device pointers (ints or None); returns (rc, offs, lens)."""
        n = len(lens)
        p = (C.c_void_p * max(n, 1))(*d_ptrs)
        ln = (C.c_size_t * max(n, 1))(*lens)
        offs = (C.c_size_t * max(n, 1))()
        olen = (C.c_size_t * max(n, 1))()
        rc = self.lib.bzx_compress_batch_device(self.ctx, n, p, ln, level, d_out, cap, offs, olen)
        return rc, list(offs[:n]), list(olen[:n])

    def batch_device(self, d_ptrs, lens, level, d_out, cap):
        rc, offs, olen = self.batch_device_raw(d_ptrs, lens, level, d_out, cap)
        self._check(rc)
        return offs, olen

    def block_info_rc(self, block=0):
        buf = (C.c_uint8 * 128)()
        return self.lib.bzx_get_block_info(self.ctx, block, buf)


__all__ = ["BatchLib", "BzxError"]
