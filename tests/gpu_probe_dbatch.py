"""Probe (not a test): batched decompression, and the one-input calls against the parent commit's; seeded synthetic
text at -9.

  python tests/gpu_probe_dbatch.py [--reps 3] [--parent-lib PATH/libbzx.so]

Cases: 4096 streams of 64 KiB, 256 streams of 1 MiB and one stream of 256 MiB through one
bzx_decompress_batch_device; one file of 64 concatenated streams of 256 KiB through bzx_decompress_batch_buffer
(count = 1).  The one-shot calls are the same decoder with count = 1, so on its own the probe only times the batch.
With --parent-lib (the parent commit built into a second directory) the one-input loops run as well, on that library
and on this one, alternated with the batch in one process: a loop of bzx_decompress_device over the first 128 / 32 / 1
streams (extrapolated to all of them), and bzx_decompress_buffer on the concatenated file.  Every library has one
context of max_blocks = 1024; every shape runs once before it is timed, then the best of --reps; times are host clock
around calls that end in a device synchronise.  The decoded bytes are checked.  Prints one line per case and a JSON
line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_ctypes import Oracle  # noqa: E402
from bzx_dbatch_ctypes import DBatchLib  # noqa: E402

MAX_BLOCKS = 1024


def best_of(sides, reps, check):
    """sides: [(label, fn)].  One checked warm-up each, then reps rounds over all of them in turn; the best times."""
    for label, fn in sides:
        fn()
        check(label)
    best = {}
    for _ in range(reps):
        for label, fn in sides:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            best[label] = min(best.get(label, dt), dt)
    return best


def compress_all(lib, d_text, count, size):
    lens = [size] * count
    cap = lib.batch_bound(lens)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    offs, olen = lib.batch_device([d_text.data_ptr() + i * size for i in range(count)], lens, 9, d_out.data_ptr(), cap)
    return d_out, offs, olen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    oracle = Oracle()
    lib = DBatchLib(max_blocks=MAX_BLOCKS)
    parent = DBatchLib(a.parent_lib, max_blocks=MAX_BLOCKS) if a.parent_lib else None
    text = oracle.synthtext(256 << 20, seed=12345)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda")
    results = {}

    def report(name, best, scale=1.0):
        r = {k + "_ms": v * 1e3 * (scale if k != "batch" else 1.0) for k, v in best.items()}
        if parent:
            r["one_shot_over_parent"] = best["one_shot"] / best["parent_one_shot"]
            r["parent_one_shot_over_batch"] = best["parent_one_shot"] * scale / best["batch"]
        results[name] = r
        print(f"{name}: " + ", ".join(f"{k} {v:.2f}" for k, v in r.items()), flush=True)

    for name, count, size, loop_n in (("4096x64KiB", 4096, 64 << 10, 128), ("256x1MiB", 256, 1 << 20, 32),
                                      ("1x256MiB", 1, 256 << 20, 1)):
        d_z, offs, olen = compress_all(lib, d_text, count, size)
        d_out = torch.zeros(count * size + 16, dtype=torch.uint8, device="cuda")
        srcs = [d_z.data_ptr() + o for o in offs]
        outs = [d_out.data_ptr() + i * size for i in range(count)]
        caps = [size] * count

        def batch():
            rc, ol, st = lib.dbatch_device_raw(srcs, olen, outs, caps)
            assert rc == 0, lib.last_error()

        def loop_of(which):
            def fn():
                n = C.c_size_t()
                for i in range(loop_n):
                    rc = which.lib.bzx_decompress_device(which.ctx, srcs[i], olen[i], outs[i], caps[i], C.byref(n))
                    assert rc == 0 and n.value == size, which.last_error()
            return fn

        def check(label):
            n = (count if label == "batch" else loop_n) * size
            assert torch.equal(d_out[:n], d_text[:n]), (name, label)
            d_out.zero_()

        sides = [("batch", batch)] + ([("one_shot", loop_of(lib)), ("parent_one_shot", loop_of(parent))] if parent else [])
        best = best_of(sides, a.reps, check)
        report(name, best, count / loop_n)                   # the loops are extrapolated to all streams
        results[name].update(loop_streams=loop_n, batch_MBps=count * size / best["batch"] / 1e6)
        del d_z, d_out
    # one pbzip2-style file: 64 streams of 256 KiB, concatenated, host buffers on both sides
    size = 256 << 10
    d_z, offs, olen = compress_all(lib, d_text, 64, size)
    zb = d_z.cpu().numpy().tobytes()
    cat = b"".join(zb[o:o + n] for o, n in zip(offs, olen))
    want = text[:64 * size]
    cap = 64 * size + (1 << 20)
    src = C.create_string_buffer(cat, len(cat))
    out = C.create_string_buffer(cap)

    def batch1():
        rc, ol, st = lib.dbatch_buffer_raw([C.addressof(src)], [len(cat)], [C.addressof(out)], [cap])
        assert rc == 0 and ol == [len(want)], lib.last_error()

    def buffer_of(which):
        def fn():
            n = C.c_size_t()
            rc = which.lib.bzx_decompress_buffer(which.ctx, cat, len(cat), out, cap, C.byref(n))
            assert rc == 0 and n.value == len(want), which.last_error()
        return fn

    def check1(label):
        assert C.string_at(out, len(want)) == want, label
        C.memset(out, 0, cap)

    sides = [("batch", batch1)] + ([("one_shot", buffer_of(lib)), ("parent_one_shot", buffer_of(parent))] if parent else [])
    report("1x(64x256KiB concatenated)", best_of(sides, a.reps, check1))
    print(json.dumps(results))
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
