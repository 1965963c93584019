"""Probe (not a test): single-process multi-device compression against the one-device call, page-locked host buffer
to page-locked host buffer.

  python tests/gpu_probe_mdev.py [--reps 3] [--parent-lib PATH/libbzx.so] [--mib 1024] [--rotate K] [--only SIDE]

Input: 1 GiB of seeded synthetic text at -9 (tests/golden/streams.json: config3_text_1GiB_l9; every side's bytes are
checked against its committed sha256 in the warm-up).  Sides: with --parent-lib bzx_compress_buffer of that library
(the parent commit built into a second directory -- the yardstick), bzx_compress_buffer of this library, and
bzx_mcompress_buffer with devices = {0}, {0,0}, {0,0,0,0} and, where the process sees them, {0,1}, {0,1,2,3} and all
devices.  Every side runs once before it is timed, then the best of --reps with the sides alternated in one process;
times are host clock around calls that return with the bytes in the caller's buffer.  Prints one line per side with
the per-entry chunks, blocks and device time of bzx_mctx_get_info, and a JSON line.  --rotate K moves the first K
sides to the end of the order (warm-up and timing), to tell an effect of the order from one of the side: a side's HIP
streams are created in its warm-up, and what was created before it may decide which hardware queues they share (a
guess: not verified).  --only SIDE (parent_buffer, buffer, mdev[0], mdev[0,0], ...) creates, warms up and times that
side alone: run once per side, each in a fresh process and with more --reps, it gives figures free of that effect; it
also prints the median.  The same form is what a rocprofv3 --kernel-trace --stats run of one side takes."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_ctypes import ROOT, BzxLib, Oracle  # noqa: E402
from bzx_mdev_ctypes import MDev, bind  # noqa: E402

MAX_BLOCKS = 260          # the blocks of one chunk of the one-shot calls (one per compute unit) + the withheld one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--rotate", type=int, default=0)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    have = torch.cuda.device_count()
    oracle = Oracle()
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "streams.json")))["streams"]["config3_text_1GiB_l9"]
    n = a.mib << 20
    check = n == g["raw_len"]
    lib = BzxLib(max_blocks=MAX_BLOCKS)
    L = bind(lib.lib)
    parent = BzxLib(a.parent_lib, max_blocks=MAX_BLOCKS) if a.parent_lib and a.only in (None, "parent_buffer") else None
    cap = n + n // 50 + 4096
    p_src, p_out = L.bzx_host_alloc(n), L.bzx_host_alloc(cap)
    assert p_src and p_out
    oracle.lib.bzo_synthtext(0x9E3779B97F4A7C15, (C.c_char * n).from_address(p_src), n)

    def one_device(which):
        which.lib.bzx_compress_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                                  C.POINTER(C.c_size_t)]

        def fn():
            ol = C.c_size_t()
            rc = which.lib.bzx_compress_buffer(which.ctx, p_src, n, 9, p_out, cap, C.byref(ol))
            assert rc == 0, rc
            return ol.value
        return fn

    sets = [(0,), (0, 0), (0, 0, 0, 0)]
    if have >= 2:
        sets.append((0, 1))
    if have >= 4:
        sets.append((0, 1, 2, 3))
    if have >= 2 and tuple(range(have)) not in sets:
        sets.append(tuple(range(have)))
    name_of = lambda d: "mdev" + str(list(d)).replace(" ", "")          # noqa: E731
    if a.only:
        sets = [d for d in sets if name_of(d) == a.only]
    mds = {d: MDev(d, max_blocks=MAX_BLOCKS) for d in sets}
    sides = ([("parent_buffer", one_device(parent))] if parent else []) + [("buffer", one_device(lib))]
    for d in sets:
        sides.append(("mdev" + str(list(d)).replace(" ", ""), lambda md=mds[d]: md.compress_ptr(p_src, n, 9, p_out, cap)))
    if a.only:
        sides = [x for x in sides if x[0] == a.only]
        assert sides, "no such side: " + a.only
    sides = sides[a.rotate % len(sides):] + sides[:a.rotate % len(sides)]
    best, every = {}, {}
    for label, fn in sides:                                   # warm-up, bytes checked
        C.memset(p_out, 0, cap)
        got = fn()
        if check:
            assert got == g["bz2_len"], (label, got)
            assert hashlib.sha256((C.c_char * got).from_address(p_out)).hexdigest() == g["bz2_sha256"], label
    for _ in range(a.reps):                                   # alternated
        for label, fn in sides:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            best[label] = min(best.get(label, dt), dt)
            every.setdefault(label, []).append(dt)
    ref = best.get("parent_buffer", best["buffer"])
    results = {"mib": a.mib, "order": [label for label, _ in sides], "checked": check, "devices_seen": have, "max_blocks": MAX_BLOCKS,
               "ms": {k: v * 1e3 for k, v in best.items()},
               "median_ms": {k: sorted(v)[len(v) // 2] * 1e3 for k, v in every.items()}, "over_yardstick": {k: v / ref for k, v in best.items()}}
    for label, _ in sides:
        line = f"{label}: {best[label] * 1e3:.1f} ms (median {results['median_ms'][label]:.1f}), {n / best[label] / 1e9:.2f} GB/s, x{best[label] / ref:.3f} of the yardstick"
        if label.startswith("mdev"):
            d = next(x for x in sets if "mdev" + str(list(x)).replace(" ", "") == label)
            i = mds[d].info()
            per = [dict(device=i.dev[e].device, chunks=i.dev[e].chunks, blocks=i.dev[e].blocks,
                        ms_device=round(i.dev[e].ms_device, 2), device_MB=round(i.dev[e].device_bytes / 1e6, 1),
                        pinned_MB=round(i.dev[e].pinned_bytes / 1e6, 2)) for e in range(len(d))]
            results[label] = dict(chunks=i.chunks, shifted=i.shifted, nblk=i.nblk, entries=per)
            line += f"; chunks {i.chunks}, shifted {i.shifted}; " + "; ".join(
                f"[{e}] dev {p['device']}: {p['chunks']} chunks, {p['blocks']} blocks, {p['ms_device']} ms" for e, p in enumerate(per))
        print(line, flush=True)
    print(json.dumps(results))
    for md in mds.values():
        md.close()
    L.bzx_host_free(p_src)
    L.bzx_host_free(p_out)
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
