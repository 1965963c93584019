"""Probe (not a test): streaming decompression against the one-shot call, host buffer to host buffer.

  python tests/gpu_probe_dstream.py [--reps 3] [--parent-lib PATH/libbzx.so] [--max-chunk BYTES]

Inputs: one stream of 256 MiB of seeded synthetic text at -9, and one file of 64 concatenated streams of 256 KiB
(DESIGN 5c).  Sides: bzx_dstream_* (everything fed in one call with final, the output taken in one buffer) and
bzx_decompress_buffer of the same library; with --parent-lib also both of that library (the parent commit built into
a second directory), alternated in one process.  Every side has one context of
max_blocks = 1024; every shape runs once before it is timed, then the best of --reps; times are host clock around
calls that return with the bytes in the caller's buffer.  The decoded bytes are checked.  Prints one line per case
and a JSON line (all_ms: every run of every side)."""
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

MAX_BLOCKS = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--max-chunk", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.init()
    oracle = Oracle()
    lib = DStreamLib(max_blocks=MAX_BLOCKS)
    parent = DStreamLib(a.parent_lib, max_blocks=MAX_BLOCKS) if a.parent_lib else None
    text = oracle.synthtext(256 << 20, seed=12345)
    one = lib.compress_buffer(text, 9)
    size = 256 << 10
    cat = b"".join(lib.compress_buffer(text[i * size:(i + 1) * size], 9) for i in range(64))
    results = {"max_blocks": MAX_BLOCKS, "max_chunk": a.max_chunk}
    for name, z, want in (("1x256MiB", one, text), ("64x256KiB concatenated", cat, text[:64 * size])):
        cap = len(want) + (1 << 20)
        src = C.create_string_buffer(z, len(z))
        out = C.create_string_buffer(cap)
        info = {}

        def stream_of(which):
            return lambda: stream(which)

        def stream(which):
            s = which.dstream(a.max_chunk)
            try:
                pos, total, done = 0, 0, 0
                while not done:
                    rc, used, made, done = s.feed_raw(C.addressof(src) + pos, len(z) - pos, True, C.addressof(out) + total,
                                                      cap - total)
                    assert rc == 0, which.last_error()
                    pos += used
                    total += made
                assert total == len(want)
                i = s.info()
                info.update(windows=i.windows, rounds=i.rounds, scans=i.scans, slabs=i.slabs, nblk=i.nblk,
                            device_MB=i.device_bytes / 1e6, pinned_MB=i.pinned_bytes / 1e6)
            finally:
                s.end()

        def buffer_of(which):
            def fn():
                n = C.c_size_t()
                rc = which.lib.bzx_decompress_buffer(which.ctx, z, len(z), out, cap, C.byref(n))
                assert rc == 0 and n.value == len(want), which.last_error()
            return fn

        sides = [("stream", stream_of(lib)), ("buffer", buffer_of(lib))]
        if parent:
            sides += [("parent_stream", stream_of(parent)), ("parent_buffer", buffer_of(parent))]
        runs = {label: [] for label, _ in sides}
        for label, fn in sides:                                   # warm-up, bytes checked
            C.memset(out, 0, cap)
            fn()
            assert C.string_at(out, len(want)) == want, (name, label)
        for _ in range(a.reps):                                   # alternated
            for label, fn in sides:
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                runs[label].append(dt)
        best = {k: min(v) for k, v in runs.items()}
        r = {k + "_ms": v * 1e3 for k, v in best.items()}
        r["all_ms"] = {k: [round(x * 1e3, 2) for x in v] for k, v in runs.items()}
        ref = best.get("parent_buffer", best["buffer"])
        r["stream_over_one_shot"] = best["stream"] / ref
        r.update(info)
        results[name] = r
        print(f"{name}: " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in best.items()) +
              f"; stream / one-shot = {best['stream'] / ref:.3f}; {info}", flush=True)
    print(json.dumps(results))
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
