"""Probe (not a test): what keeping the block index costs a compression call, and what it saves.

  python tests/gpu_probe_cindex.py [--reps 3] [--build-reps N] [--part all|one|batch] [--parent-lib PATH] [--mib 256]
                                   [--inputs 4096]

Two workloads, -9, seeded synthetic text: one input of 256 MiB through bzx_compress_device, and a batch of 4096 inputs of
64 KiB through bzx_compress_batch_device.  Three sides each, alternated in one process after a warm-up of every side,
best of --reps: compression with keeping off, compression with keeping on, and compression with keeping off followed by
bzx_index_build_buffer of the output (one call per stream: the path that keeping replaces; for the batch that is 4096
calls of some 50 ms each, so --build-reps sets the passes of that side alone, and a line of progress is printed every
512 calls).  --parent-lib: another build of the library (the parent commit's) times the first side too.  Times are host clock around calls that end in a device
synchronise.  Checked on the way: the bytes with keeping on are the bytes with keeping off, and the compressor's entries
are the decoder's (for the batch: of every 64th stream before the timed passes, of all of them in the first timed pass
of the third side).  Prints one line per workload and a JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_batch_ctypes import BatchLib  # noqa: E402
from bzx_cindex_ctypes import CIndexLib  # noqa: E402
from bzx_ctypes import Oracle  # noqa: E402

MAX_BLOCKS = 512            # a 256 MiB input at -9 is 299 blocks; the batch then takes 8 device rounds


def best(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--build-reps", type=int, default=None, help="passes of compress-then-index (default: --reps)")
    ap.add_argument("--part", default="all", choices=["all", "one", "batch"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--inputs", type=int, default=4096)
    a = ap.parse_args()
    build_reps = a.reps if a.build_reps is None else a.build_reps
    torch.cuda.init()
    oracle = Oracle()
    off = CIndexLib(max_blocks=MAX_BLOCKS)
    on = CIndexLib(max_blocks=MAX_BLOCKS)
    assert on.keep_index(1) == 0
    parent = BatchLib(a.parent_lib, max_blocks=MAX_BLOCKS) if a.parent_lib else None
    total = max(a.mib << 20, a.inputs * (64 << 10))
    text = oracle.synthtext(total, seed=12345)
    d_in = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda")
    results = {}

    if a.part != "batch":
        probe_one(a, off, on, parent, d_in, build_reps, results)
    if a.part != "one":
        probe_batch(a, off, on, parent, d_in, build_reps, results)
    print(json.dumps(results))
    for lib in (off, on, parent):
        if lib:
            lib.close()


def probe_one(a, off, on, parent, d_in, build_reps, results):
    size = a.mib << 20
    cap = size + size // 50 + 4096
    d_out = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def one(lib, k=0):
        return lib.compress_device(d_in.data_ptr(), size, 9, d_out[k].data_ptr(), cap)

    def one_then_build():
        n = one(off)
        z = d_out[0][:n].cpu().numpy().tobytes()
        return off.index_build_bytes(z)

    n_off, n_on = one(off, 0), one(on, 1)                          # warm-up and checks
    assert n_off == n_on and torch.equal(d_out[0][:n_off], d_out[1][:n_on]), "keeping changed the compressed bytes"
    rc, entries, info = on.compress_get_index()
    assert rc == 0 and (entries, info) == one_then_build(), "the compressor's index is not the decoder's"
    if parent:
        assert one(parent, 1) == n_off and torch.equal(d_out[0][:n_off], d_out[1][:n_off])
    t = {"off": [], "on": [], "off_then_build": [], "parent_off": []}
    for k in range(a.reps):                                         # sides alternated
        t["off"] += best(lambda: one(off), 1)
        t["on"] += best(lambda: one(on, 1), 1)
        if parent:
            t["parent_off"] += best(lambda: one(parent, 1), 1)
        if k < build_reps:
            t["off_then_build"] += best(one_then_build, 1)
    results["1x%dMiB" % a.mib] = r = {k: round(min(v) * 1e3, 2) for k, v in t.items() if v}
    r.update(blocks=info[2], all_ms={k: [round(x * 1e3, 2) for x in v] for k, v in t.items() if v})
    print(f"1 x {a.mib} MiB, {info[2]} blocks: " + "  ".join(f"{k} {v} ms" for k, v in r.items() if k in t), flush=True)
    del d_out
    torch.cuda.empty_cache()


def probe_batch(a, off, on, parent, d_in, build_reps, results):
    count, each = a.inputs, 64 << 10
    lens = [each] * count
    ptrs = [d_in.data_ptr() + i * each for i in range(count)]
    cap = off.batch_bound(lens)
    d_out = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def batch(lib, k=0):
        return lib.batch_device(ptrs, lens, 9, d_out[k].data_ptr(), cap)

    def batch_then_build(step=1):
        offs, olen = batch(off)
        raw = d_out[0].cpu().numpy().tobytes()
        out = []
        for i in range(0, count, step):
            out.append(off.index_build_bytes(raw[offs[i]:offs[i] + olen[i]])[0])
            if step == 1 and (i + 1) % 512 == 0:
                print(f"  compress-then-index: {i + 1} of {count} streams", flush=True)
        return out

    (offs, olen), (offs2, olen2) = batch(off, 0), batch(on, 1)
    assert (offs, olen) == (offs2, olen2) and torch.equal(d_out[0], d_out[1]), "keeping changed the compressed bytes"
    rc, slices = on.batch_get_index()
    assert rc == 0 and slices[::64] == batch_then_build(64), "the compressor's index is not the decoder's"
    if parent:
        assert batch(parent, 1) == (offs, olen) and torch.equal(d_out[0], d_out[1])
    t = {"off": [], "on": [], "off_then_build": [], "parent_off": []}
    built = []
    for k in range(a.reps):
        t["off"] += best(lambda: batch(off), 1)
        t["on"] += best(lambda: batch(on, 1), 1)
        if parent:
            t["parent_off"] += best(lambda: batch(parent, 1), 1)
        if k < build_reps:
            t["off_then_build"] += best(lambda: built.append(batch_then_build()), 1)
            assert built.pop() == slices, "the compressor's index is not the decoder's"
    results["%dx64KiB" % count] = r = {k: round(min(v) * 1e3, 2) for k, v in t.items() if v}
    r.update(blocks=sum(len(s) // 40 for s in slices), all_ms={k: [round(x * 1e3, 2) for x in v] for k, v in t.items() if v})
    print(f"{count} x 64 KiB, {r['blocks']} blocks: " + "  ".join(f"{k} {v} ms" for k, v in r.items() if k in t), flush=True)


if __name__ == "__main__":
    main()
