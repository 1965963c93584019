"""ctypes bindings of the batched range reads (include/bzx.h: bzx_index_spans, bzx_decompress_ranges_*,
bzx_stage_gather), used by the tests of the batched range reads and their probe.  RangesLib is the RangeLib of
bzx_range_ctypes.py with those functions bound."""
import ctypes as C

from bzx_ctypes import LIB_PATH
from bzx_range_ctypes import IndexEntry, RangeLib


class Piece(C.Structure):
    _fields_ = [("p", C.c_void_p), ("base", C.c_uint64), ("len", C.c_uint64)]


assert C.sizeof(Piece) == 24

U64P, SZP = C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)


def u64(values):
    return (C.c_uint64 * max(len(values), 1))(*values)


class RangesResult:
    """What one bzx_decompress_ranges_* call left: rc, need, out_offs, gots, status, and (for _buffer) the whole output
    buffer.  data(i): the bytes of range i."""

    def __init__(self, rc, need, out_offs, gots, status, room):
        self.rc, self.need, self.out_offs, self.gots, self.status, self.room = rc, need, out_offs, gots, status, room

    def data(self, i):
        return self.room[self.out_offs[i]:self.out_offs[i] + self.gots[i]]


class RangesLib(RangeLib):
    def __init__(self, path=LIB_PATH, device=0, max_blocks=16):
        super().__init__(path, device, max_blocks)
        L = self.lib
        L.bzx_index_spans.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, U64P, U64P, U64P, U64P, C.c_uint32, C.POINTER(C.c_uint32)]
        for fn in (L.bzx_decompress_ranges_device, L.bzx_decompress_ranges_buffer):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, U64P, U64P, C.c_void_p,
                           C.c_size_t, SZP, SZP, C.POINTER(C.c_int), SZP]
        L.bzx_stage_gather.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, U64P, U64P, U64P, C.c_void_p, C.c_size_t]
        L.bzx_stage_gather_time.argtypes = L.bzx_stage_gather.argtypes + [C.c_uint32, C.POINTER(C.c_float)]

    def spans(self, entries, n, ranges, cap=None):
        """bzx_index_spans -> (rc, [(base, len)], pieces needed)"""
        cap = 2 * len(ranges) + 4 if cap is None else cap
        bases, lens, np = u64([0] * cap), u64([0] * cap), C.c_uint32(12345)
        rc = self.lib.bzx_index_spans(entries, n, len(ranges), u64([r[0] for r in ranges]), u64([r[1] for r in ranges]),
                                      bases, lens, cap, C.byref(np))
        return rc, [(bases[i], lens[i]) for i in range(min(cap, np.value))], np.value

    def ranges_raw(self, fn, pieces, entries, n, ranges, out, cap):
        """One call of fn (the _device or the _buffer form) with pieces = [(address, base, len)] -> RangesResult without
        the output bytes."""
        count = len(ranges)
        pc = (Piece * max(len(pieces), 1))(*[Piece(p, b, ln) for p, b, ln in pieces])
        offs, gots = (C.c_size_t * max(count, 1))(*[77] * max(count, 1)), (C.c_size_t * max(count, 1))(*[77] * max(count, 1))
        status, need = (C.c_int * max(count, 1))(*[77] * max(count, 1)), C.c_size_t(12345)
        rc = fn(self.ctx, pc, len(pieces), entries, n, count, u64([r[0] for r in ranges]), u64([r[1] for r in ranges]), out,
                cap, offs, gots, status, C.byref(need))
        return RangesResult(rc, need.value, list(offs[:count]), list(gots[:count]), list(status[:count]), None)

    def ranges_buffer(self, z, pieces, entries, n, ranges, cap=None, fill=0xA5):
        """bzx_decompress_ranges_buffer.  pieces: [(base, len)] of z, the whole file (None: one piece that is the whole
        file); each piece is handed over in a buffer of its own."""
        pieces = [(0, len(z))] if pieces is None else pieces
        bufs = [C.create_string_buffer(bytes(z[b:b + ln]), max(ln, 1)) for b, ln in pieces]
        if cap is None:
            total = entries[n - 1].out_off + entries[n - 1].out_len if n else 0
            cap = sum(max(0, min(total, o + w) - o) for o, w in ranges)
        out = C.create_string_buffer(bytes([fill]) * max(cap, 1), max(cap, 1))
        r = self.ranges_raw(self.lib.bzx_decompress_ranges_buffer, [(C.addressof(bf), b, ln) for bf, (b, ln) in zip(bufs, pieces)],
                            entries, n, ranges, C.addressof(out), cap)
        r.room = out.raw[:cap]
        return r

    def stage_gather(self, src, slices, out):
        """bzx_stage_gather: slices = [(src_off, dst_off, len)], out = the pre-filled destination -> (rc, out afterwards)"""
        buf = C.create_string_buffer(bytes(out), max(len(out), 1))
        rc = self.lib.bzx_stage_gather(self.ctx, bytes(src), len(src), len(slices), u64([s[0] for s in slices]),
                                       u64([s[1] for s in slices]), u64([s[2] for s in slices]), buf, len(out))
        return rc, buf.raw[:len(out)]


__all__ = ["RangesLib", "RangesResult", "Piece", "IndexEntry"]
