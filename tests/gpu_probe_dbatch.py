"""Probe (not a test): batched decompression against the one-input decoders, seeded synthetic text at -9.

  python tests/gpu_probe_dbatch.py [--reps 3]

Cases: 4096 streams of 64 KiB and 256 streams of 1 MiB (one bzx_decompress_batch_device against a loop of
bzx_decompress_device over the first 128 / 32 streams, extrapolated to all of them); one file of 64 concatenated
streams of 256 KiB (count = 1 through bzx_decompress_batch_buffer against bzx_decompress_buffer); one stream of 256 MiB
(count = 1 against bzx_decompress_device).  The streams are made by the batch compressor.  One context
(max_blocks = 1024) serves both sides; every shape runs once before it is timed, then the best of --reps; times are
host clock around calls that end in a device synchronise.  The decoded bytes are checked.  Prints one line per case and
a JSON line."""
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


def best(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def compress_all(lib, d_text, count, size):
    lens = [size] * count
    cap = lib.batch_bound(lens)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    offs, olen = lib.batch_device([d_text.data_ptr() + i * size for i in range(count)], lens, 9, d_out.data_ptr(), cap)
    return d_out, offs, olen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.init()
    oracle = Oracle()
    lib = DBatchLib(max_blocks=MAX_BLOCKS)
    L = lib.lib
    text = oracle.synthtext(256 << 20, seed=12345)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda")
    results = {}
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

        def loop():
            n = C.c_size_t()
            for i in range(loop_n):
                rc = L.bzx_decompress_device(lib.ctx, srcs[i], olen[i], outs[i], caps[i], C.byref(n))
                assert rc == 0 and n.value == size, lib.last_error()

        t_b = best(batch, a.reps)
        d_out.zero_()
        batch()
        assert torch.equal(d_out[:count * size], d_text[:count * size]), name
        t_l = best(loop, a.reps) * count / loop_n
        d_out.zero_()
        loop()
        assert torch.equal(d_out[:loop_n * size], d_text[:loop_n * size]), name
        results[name] = dict(batch_ms=t_b * 1e3, loop_ms=t_l * 1e3, loop_extrapolated=loop_n < count,
                             speedup=t_l / t_b, batch_MBps=count * size / t_b / 1e6)
        print(f"{name}: batch {t_b * 1e3:.2f} ms, loop {t_l * 1e3:.2f} ms"
              f"{' (extrapolated from ' + str(loop_n) + ')' if loop_n < count else ''}, {t_l / t_b:.2f}x", flush=True)
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

    def single():
        n = C.c_size_t()
        rc = L.bzx_decompress_buffer(lib.ctx, cat, len(cat), out, cap, C.byref(n))
        assert rc == 0 and n.value == len(want), lib.last_error()

    t_b = best(batch1, a.reps)
    assert C.string_at(out, len(want)) == want
    t_s = best(single, a.reps)
    assert C.string_at(out, len(want)) == want
    results["1x(64x256KiB concatenated)"] = dict(batch_ms=t_b * 1e3, buffer_ms=t_s * 1e3, speedup=t_s / t_b)
    print(f"64x256KiB concatenated: batch {t_b * 1e3:.2f} ms, bzx_decompress_buffer {t_s * 1e3:.2f} ms, "
          f"{t_s / t_b:.2f}x", flush=True)
    print(json.dumps(results))
    lib.close()


if __name__ == "__main__":
    main()
