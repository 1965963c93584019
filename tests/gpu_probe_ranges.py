"""Probe (not a test): what the batched range read buys.

  python tests/gpu_probe_ranges.py [--reps 3] [--parent-lib PATH/libbzx.so] [--part compare,one,gather,trace]

compare  1,000 seeded reads of 4 KiB and of 64 KiB from 64 MiB of seeded text at -9: ONE bzx_decompress_ranges_buffer
         call (the pieces of bzx_index_spans, cut out of the file before the clock starts) against a loop of 1,000
         bzx_decompress_range_buffer calls of --parent-lib (the parent commit built into a second directory; without it,
         this library's own single call).
one      this library's single call against the single call of --parent-lib (single_call) and against count = 1 of the
         batched call, all through _buffer with the span alone: 64 KiB inside one block, 1 byte, 64 KiB across a block
         border.  The gate: the single call's best is not above the parent's best by more than the spread (max - min over
         the runs of any side) seen in that same run.
gather   the gather kernel alone under HIP events (bzx_stage_gather_time): 1,000 slices of 4 KiB at seeded odd
         addresses, and one slice of 45 MB, in GB/s.
trace    one batched call of the 4 KiB list, for rocprofv3 --kernel-trace --stats (no timing).
Every shape runs once before it is timed, then the best of --reps with the sides alternated in one process; the bytes
are checked.  Prints one line per case and a JSON line."""
import argparse
import ctypes as C
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_ctypes import Oracle  # noqa: E402
from bzx_range_ctypes import RangeLib  # noqa: E402
from bzx_ranges_ctypes import Piece, RangesLib, u64  # noqa: E402
from gpu_probe_range import alternate, report  # noqa: E402


def batched(lib, z, entries, n, ranges):
    """-> (fn, the output buffer, out_offs): one bzx_decompress_ranges_buffer call over the pieces of bzx_index_spans."""
    rc, pieces, np = lib.spans(entries, n, ranges)
    assert rc == 0
    bufs = [C.create_string_buffer(z[b:b + ln], ln) for b, ln in pieces]
    pc = (Piece * len(pieces))(*[Piece(C.addressof(bf), b, ln) for bf, (b, ln) in zip(bufs, pieces)])
    count = len(ranges)
    need = sum(w for _, w in ranges)
    out = C.create_string_buffer(need)
    offs, wants = u64([o for o, _ in ranges]), u64([w for _, w in ranges])
    oo, gg, st, nd = (C.c_size_t * count)(), (C.c_size_t * count)(), (C.c_int * count)(), C.c_size_t()

    def fn():
        rc = lib.lib.bzx_decompress_ranges_buffer(lib.ctx, pc, len(pieces), entries, n, count, offs, wants, C.addressof(out), need,
                                                  oo, gg, st, C.byref(nd))
        assert rc == 0 and nd.value == need, lib.last_error()
    fn.keep = (bufs, pc)
    return fn, out, oo, sum(ln for _, ln in pieces), len(pieces)


def looped(side, z, entries, n, ranges):
    """-> (fn, the output buffer): a loop of bzx_decompress_range_buffer calls, the whole file at hand (the library uploads
    each range's span alone)."""
    need = sum(w for _, w in ranges)
    out = C.create_string_buffer(need)
    src = C.create_string_buffer(z, len(z))
    got = C.c_size_t()
    f = side.lib.bzx_decompress_range_buffer

    def fn():
        at = 0
        for off, w in ranges:
            rc = f(side.ctx, C.addressof(src), len(z), 0, entries, n, off, w, C.addressof(out) + at, C.byref(got))
            assert rc == 0 and got.value == w, side.last_error()
            at += w
    return fn, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--part", default="compare,one,gather")
    a = ap.parse_args()
    parts = set(a.part.split(","))
    torch.cuda.init()
    oracle = Oracle()
    results = {"parent_lib": bool(a.parent_lib)}
    lib = RangesLib(max_blocks=16)
    maker = RangeLib(max_blocks=16)
    parent = RangeLib(a.parent_lib, max_blocks=16) if a.parent_lib else lib
    side = "parent_loop" if a.parent_lib else "own_loop"

    if parts & {"compare", "one", "trace"}:
        raw = oracle.synthtext(64 << 20, seed=12345)
        z = maker.compress_buffer(raw, 9)
        rc, entries, info = lib.index_build(z)
        assert rc == 0, lib.last_error()
        n = info.nblk
        rnd = random.Random(7)
        for size in (4 << 10, 64 << 10):
            ranges = [(rnd.randrange(0, len(raw) - size), size) for _ in range(1000)]
            want = b"".join(raw[o:o + w] for o, w in ranges)
            fb, ob, _, piece_bytes, npieces = batched(lib, z, entries, n, ranges)
            fb()
            assert ob.raw == want
            nblk = lib.stats().nblk
            if "trace" in parts and size == 4 << 10:
                fb()
            if "compare" not in parts:
                continue
            fl, ol = looped(parent, z, entries, n, ranges)
            fl()
            assert ol.raw == want
            t = alternate([("batched", fb), (side, fl)], a.reps)
            r = report(f"1000 reads of {size >> 10} KiB ({nblk} distinct blocks of {n}, {npieces} pieces, {piece_bytes} bytes read)", t, results)
            r["loop_over_batched"] = min(t[side]) / min(t["batched"])
            r["gate_batched_faster"] = bool(min(t["batched"]) < min(t[side]))
            print(f"  loop / batched = {r['loop_over_batched']:.1f}; gate (batched faster): {r['gate_batched_faster']}", flush=True)

        if "one" in parts:
            e = entries[n // 2]
            shapes = [("64 KiB of one block", e.out_off + e.out_len // 2, 65536), ("1 byte", e.out_off + e.out_len // 2, 1),
                      ("64 KiB across a block border", e.out_off - 32768, 65536)]
            for name, off, w in shapes:
                fb, ob, _, _, _ = batched(lib, z, entries, n, [(off, w)])
                rc, first, count, lo, hi = lib.span(entries, n, off, w)
                span = C.create_string_buffer(z[lo:hi], hi - lo)

                def single(sd):
                    o1, got = C.create_string_buffer(w), C.c_size_t()

                    def fn():
                        rc = sd.lib.bzx_decompress_range_buffer(sd.ctx, C.addressof(span), hi - lo, lo, entries, n, off, w,
                                                                C.addressof(o1), C.byref(got))
                        assert rc == 0 and got.value == w, sd.last_error()
                    return fn, o1
                own, oo = single(lib)
                par, op = single(parent)
                fb()
                own()
                par()
                assert ob.raw == oo.raw == op.raw == raw[off:off + w]
                t = alternate([("own_single_call", own), ("single_call", par), ("count_1", fb)], a.reps)
                r = report(f"the single call against the parent's and count = 1, {name} ({count} blocks)", t, results)
                spread = max(max(v) - min(v) for v in t.values())
                r["gate_not_slower_beyond_spread"] = bool(min(t["own_single_call"]) <= min(t["single_call"]) + spread)
                print(f"  gate (own single call not slower beyond the spread of {spread * 1e3:.3f} ms): {r['gate_not_slower_beyond_spread']}",
                      flush=True)

    if "gather" in parts:
        rnd = random.Random(9)
        src = oracle.randbytes(48 << 20)
        cases = [("1000 slices of 4 KiB", [(rnd.randrange(0, len(src) - 4096), 4096) for _ in range(1000)]),
                 ("one slice of 45 MB", [(5, 45_000_000)])]
        for name, sl in cases:
            at, slices = 3, []
            for so, ln in sl:
                slices.append((so, at, ln))
                at += ln
            out = C.create_string_buffer(at + 8)
            ms = C.c_float()
            rc = lib.lib.bzx_stage_gather_time(lib.ctx, src, len(src), len(slices), u64([s[0] for s in slices]),
                                               u64([s[1] for s in slices]), u64([s[2] for s in slices]), out, at + 8,
                                               a.reps + 1, C.byref(ms))
            assert rc == 0, lib.last_error()
            assert out.raw[3:at] == b"".join(src[so:so + ln] for so, _, ln in slices)
            gbs = (at - 3) / (ms.value * 1e-3) / 1e9
            results[f"gather alone, {name}"] = {"best_ms": ms.value, "GB_per_s_copied": gbs}
            print(f"gather alone, {name}: best {ms.value:.4f} ms, {gbs:.1f} GB/s copied (read + written: twice that)", flush=True)
    print(json.dumps(results))
    lib.close()
    maker.close()
    if a.parent_lib:
        parent.close()


if __name__ == "__main__":
    main()
