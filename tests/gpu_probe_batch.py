"""Probe (not a test): batched compression against a loop of bzx_compress_device, -9, seeded synthetic text.

  python tests/gpu_probe_batch.py [--reps 3] [--skip-gib]

Cases: 4096 x 64 KiB, 256 x 1 MiB, 1 x 1 GiB.  One context (max_blocks = 1024) serves both sides; every shape is run
once before it is timed; times are host clock around work that ends in a device synchronise (both entry points
synchronise before they return).  Prints one line per case and a JSON line with MB/s and device rounds."""
import argparse
import bz2
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_batch_ctypes import BatchLib  # noqa: E402
from bzx_ctypes import Oracle  # noqa: E402

MAX_BLOCKS = 1024


def rounds_of(nblk_each, R):
    """Device rounds of whole inputs with at most R blocks each (the library's greedy rule)."""
    rounds, cur = 0, None
    for n in nblk_each:
        if cur is None or cur + n > R:
            rounds, cur = rounds + 1, 0
        cur += n
    return rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-gib", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    oracle = Oracle()
    lib = BatchLib(max_blocks=MAX_BLOCKS)
    total = 1 << 30
    text = oracle.synthtext(total, seed=12345)
    d_in = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda")
    cases = [("4096x64KiB", 4096, 64 << 10), ("256x1MiB", 256, 1 << 20)]
    if not a.skip_gib:
        cases.append(("1x1GiB", 1, 1 << 30))
    results = {}
    for name, count, size in cases:
        lens = [size] * count
        ptrs = [d_in.data_ptr() + i * size for i in range(count)]
        cap = lib.batch_bound(lens)
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        one_cap = size + size // 50 + 4096
        d_one = torch.zeros(one_cap, dtype=torch.uint8, device="cuda")

        def batch():
            return lib.batch_device(ptrs, lens, 9, d_out.data_ptr(), cap)

        def loop():
            return [lib.compress_device(p, size, 9, d_one.data_ptr(), one_cap) for p in ptrs]

        offs, olen = batch()                                    # warm-up of every shape, and a check
        st = lib.stats()
        nblk = st.nblk
        for i in sorted({0, count - 1}):                       # each stream is what bzx_compress_device makes
            k = lib.compress_device(ptrs[i], size, 9, d_one.data_ptr(), one_cap)
            got = d_out[offs[i]:offs[i] + olen[i]].cpu().numpy().tobytes()
            assert got == d_one[:k].cpu().numpy().tobytes(), (name, i)
            if size <= (1 << 20):
                assert got == bz2.compress(text[i * size:(i + 1) * size], 9), (name, i)
        loop()
        tb, tl = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch()
            t1 = time.perf_counter()
            loop()
            t2 = time.perf_counter()
            tb.append(t1 - t0)
            tl.append(t2 - t1)
        mb = count * size / 1e6
        b, l = min(tb), min(tl)
        R = max(MAX_BLOCKS, nblk // count)
        r = {"inputs": count, "bytes_each": size, "blocks": nblk, "rounds": rounds_of([nblk // count] * count, R),
             "batch_ms": round(b * 1e3, 2), "loop_ms": round(l * 1e3, 2), "batch_MBps": round(mb / b, 1),
             "loop_MBps": round(mb / l, 1), "speedup": round(l / b, 2),
             "batch_ms_all": [round(x * 1e3, 2) for x in tb], "loop_ms_all": [round(x * 1e3, 2) for x in tl]}
        results[name] = r
        print(f"{name}: batch {r['batch_ms']} ms ({r['batch_MBps']} MB/s, {r['rounds']} round(s), {nblk} blocks)  "
              f"loop {r['loop_ms']} ms ({r['loop_MBps']} MB/s)  x{r['speedup']}", flush=True)
        del d_out, d_one
        torch.cuda.empty_cache()
    print(json.dumps(results))
    lib.close()


if __name__ == "__main__":
    main()
