"""Probe (not a test): what a range read costs, and what the many-lane inverse-BWT walk buys.

  python tests/gpu_probe_range.py [--reps 3] [--parent-lib PATH/libbzx.so] [--part one,walk,index,trace]

one    a range read of 1 byte and of 64 KiB from the middle of 64 MiB of seeded text at -9, the span already on the
       device (bzx_decompress_range_device), against bzx_decompress_device of --parent-lib (the parent commit built
       into a second directory; without it, this library's own one-shot call, which is no yardstick) on a one-block
       stream made of that same block.  The gate: the range read is not slower than the parent beyond the spread seen
       across the runs.
walk   the walk alone: wide = 1 against wide = 0 for one block and for 299 copies of it side by side, 900,000 bytes of
       text, of random bytes and of u^k with a 30,011-byte unit.  bzx_stage_ibwt_time: the launchers of either walk
       (scatter, pack, walk; the checkpoint pass of the many-lane one) between two HIP events, nothing else.
index  bzx_index_build_buffer of one stream of 256 MiB of text at -9 against the parent's bzx_dstream_* decode of it.
trace  one 64 KiB range read and one bzx_stage_ibwt each way, for rocprofv3 --kernel-trace --stats (no timing).
Every shape runs once before it is timed, then the best of --reps with the sides alternated in one process; the bytes
are checked.  Prints one line per case and a JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_ctypes import Oracle  # noqa: E402
from bzx_dstream_ctypes import DStreamLib  # noqa: E402
from bzx_range_ctypes import RangeLib  # noqa: E402


def alternate(sides, reps):
    """sides: [(label, fn)]; one warm-up each, then reps rounds alternated -> {label: [seconds]}"""
    for _, fn in sides:
        fn()
    times = {label: [] for label, _ in sides}
    for _ in range(reps):
        for label, fn in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[label].append(time.perf_counter() - t0)
    return times


def report(name, times, results):
    r = {k: {"best_ms": min(v) * 1e3, "worst_ms": max(v) * 1e3} for k, v in times.items()}
    results[name] = r
    print(f"{name}: " + ", ".join(f"{k} best {min(v) * 1e3:.3f} ms (worst {max(v) * 1e3:.3f})" for k, v in times.items()), flush=True)
    return r


def one_block_stream(z, e):
    """The .bz2 made of the block of entry e alone: BZh9, the block's bits, the end-of-stream marker, its CRC."""
    lo, hi = e.bit // 8, (e.bit + e.img_bits + 7) // 8
    v = int.from_bytes(z[lo:hi], "big") >> ((hi * 8) - (e.bit + e.img_bits))
    v &= (1 << e.img_bits) - 1
    bits = 32 + e.img_bits + 80
    s = (int.from_bytes(b"BZh9", "big") << (e.img_bits + 80)) | (v << 80) | (0x177245385090 << 32) | e.crc
    pad = -bits % 8
    return (s << pad).to_bytes((bits + pad) // 8, "big")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--part", default="one,walk,index")
    a = ap.parse_args()
    parts = set(a.part.split(","))
    a_reps = a.reps
    torch.cuda.init()
    oracle = Oracle()
    results = {"parent_lib": bool(a.parent_lib)}
    lib = RangeLib(max_blocks=16)
    maker = RangeLib(max_blocks=16)
    parent = DStreamLib(a.parent_lib, max_blocks=16) if a.parent_lib else lib

    if parts & {"one", "trace"}:
        raw = oracle.synthtext(64 << 20, seed=12345)
        z = maker.compress_buffer(raw, 9)
        rc, entries, info = lib.index_build(z)
        assert rc == 0, lib.last_error()
        n = info.nblk
        e = entries[n // 2]
        mid = e.out_off + e.out_len // 2
        rc, first, count, lo, hi = lib.span(entries, n, mid, 65536)
        assert rc == 0 and count == 1
        d_span = torch.frombuffer(bytearray(z[lo:hi]), dtype=torch.uint8).cuda()
        d_out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        one = one_block_stream(z, e)
        d_one = torch.frombuffer(bytearray(one), dtype=torch.uint8).cuda()
        d_blk = torch.empty(e.out_len + 64, dtype=torch.uint8, device="cuda")
        block = raw[e.out_off:e.out_off + e.out_len]

        def rng(w):
            def fn():
                rc, got = lib.range_device_raw(d_span.data_ptr(), hi - lo, lo, entries, n, mid, w, d_out.data_ptr())
                assert rc == 0 and got == w, lib.last_error()
            return fn

        def one_shot():
            ol = C.c_size_t()
            rc = parent.lib.bzx_decompress_device(parent.ctx, d_one.data_ptr(), len(one), d_blk.data_ptr(), e.out_len, C.byref(ol))
            assert rc == 0 and ol.value == e.out_len, parent.last_error()

        rng(65536)()
        torch.cuda.synchronize()
        assert d_out[:65536].cpu().numpy().tobytes() == raw[mid:mid + 65536]
        one_shot()
        torch.cuda.synchronize()
        assert d_blk[:e.out_len].cpu().numpy().tobytes() == block
        if "one" in parts:
            side = "parent_one_shot" if a.parent_lib else "own_one_shot"
            t = alternate([("range_1B", rng(1)), ("range_64KiB", rng(65536)), (side, one_shot)], a.reps)
            r = report(f"one block of {e.out_len} bytes", t, results)
            spread = max(max(v) - min(v) for v in t.values())
            gate = min(t["range_64KiB"]) <= min(t[side]) + spread
            r["gate_not_slower_than_parent"] = bool(gate) if a.parent_lib else None
            print(f"  gate (range read not slower than {side} beyond the spread of {spread * 1e3:.3f} ms): {gate}", flush=True)

    if parts & {"walk", "trace"}:
        n = 900_000
        unit = oracle.synthtext(30_011, seed=7)
        imgs = [("text", oracle.synthtext(n, seed=5)), ("random bytes", oracle.randbytes(n)), ("u^k, unit 30,011", unit * (n // len(unit)))]
        wlib = RangeLib(max_blocks=299) if "walk" in parts else lib
        for name, img in imgs if "walk" in parts else imgs[:1]:
            L, orig = lib.stage_bwt(img)[:2]
            wa, wb = lib.stage_ibwt(L, orig, 0, raw_cap=len(img) + 64), lib.stage_ibwt(L, orig, 1, raw_cap=len(img) + 64)
            assert wa == wb and wb[0] == img, name                            # the bytes, before anything is timed
            if "walk" not in parts:
                continue
            for copies in (1, 299):
                # the launchers alone under HIP events (bzx_stage_ibwt_time): warm-up, then the best of reps, alternated
                t = {"wide": [], "one_lane": []}
                for rep in range(a_reps + 1):
                    for label, wide in (("wide", 1), ("one_lane", 0)):
                        ms = C.c_float()
                        rc = wlib.lib.bzx_stage_ibwt_time(wlib.ctx, L, len(L), orig, wide, copies, 1, C.byref(ms))
                        assert rc == 0, wlib.last_error()
                        if rep:
                            t[label].append(ms.value / 1e3)
                r = report(f"walk alone (kernels, HIP events), {name}, {copies} x {len(img)} bytes", t, results)
                r["one_lane_over_wide"] = min(t["one_lane"]) / min(t["wide"])
                print(f"  one-lane / wide = {r['one_lane_over_wide']:.1f}", flush=True)
        if wlib is not lib:
            wlib.close()

    if "index" in parts:
        raw = oracle.synthtext(256 << 20, seed=12345)
        z = maker.compress_buffer(raw, 9)
        big = RangeLib(max_blocks=320)
        pbig = DStreamLib(a.parent_lib, max_blocks=320) if a.parent_lib else big
        rc, entries, info = big.index_build(z)
        assert rc == 0 and info.out_bytes == len(raw), big.last_error()
        n = info.nblk
        out = C.create_string_buffer(len(raw) + 64)
        src = C.create_string_buffer(z, len(z))

        def index():
            rc, _, i = big.index_build(z)
            assert rc == 0 and i.nblk == n

        def stream():
            s = pbig.dstream(0)
            try:
                pos, total, done = 0, 0, 0
                while not done:
                    rc, used, made, done = s.feed_raw(C.addressof(src) + pos, len(z) - pos, True, C.addressof(out) + total,
                                                      len(raw) + 64 - total)
                    assert rc == 0, pbig.last_error()
                    pos += used
                    total += made
                assert total == len(raw)
            finally:
                s.end()
        stream()
        assert C.string_at(out, len(raw)) == raw
        side = "parent_dstream" if a.parent_lib else "own_dstream"
        t = alternate([("index_build", index), (side, stream)], a.reps)
        r = report(f"index build of the 256 MiB stream ({n} blocks)", t, results)
        r["index_over_dstream"] = min(t["index_build"]) / min(t[side])
        print(f"  index build / stream decode = {r['index_over_dstream']:.3f}", flush=True)
        big.close()
        if a.parent_lib:
            pbig.close()
    print(json.dumps(results))
    lib.close()
    maker.close()
    if a.parent_lib:
        parent.close()


if __name__ == "__main__":
    main()
