"""Probe (not a test): what a find costs the index pass.

  python tests/gpu_probe_find.py [--reps 5] [--mib 1024] [--slabs 256] [--parent-lib PATH] [--parent-first]
                                 [--zeros-mib 256]

Two inputs.  Text: --mib MiB of seeded synthetic text compressed at -9 by the library.  Zeros: --zeros-mib MiB of zero
bytes at level 9 (three passes per 100 MiB: a block expands to 46.62 MB), where an all-zero pattern hits at every position.
Sides, alternated in one process after a warm-up of every side, host clock around calls that end in a device
synchronisation, every run listed with its best and its spread (max - min):
  text   parent_off  bzx_index_build_buffer of another build of the library (--parent-lib: the parent commit's)
         off         the same call of this build
         rare        bzx_find_buffer with a 16-byte pattern cut from the text (its hits are checked against bytes.find)
         common      bzx_find_buffer with "e " and cap_hits = 0: counted only
  zeros  off         bzx_index_build_buffer
         every4      bzx_find_buffer, four zero bytes, cap_hits = 0: every position a hit, no verify beyond the prefix
         every16     ... sixteen zero bytes: every verify runs to its end
         every4_list ... four zero bytes and cap_hits = 4 x window_hits: the emit windows
--parent-first creates the parent build's context before this build's (the default is the other order): the index pass
is a chase through device memory, and which context allocates first has shown in its time.
Prints one line per side and a JSON line."""
import argparse
import bz2
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import find_cases as FC  # noqa: E402
from bzx_ctypes import Oracle  # noqa: E402
from bzx_find_ctypes import FindLib, geometry  # noqa: E402
from bzx_range_ctypes import RangeLib  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def alternate(sides, reps):
    for fn in sides.values():                                           # warm-up
        assert fn()[0] == 0
    t = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            dt, out = clock(fn)
            assert out[0] == 0
            t[k].append(dt * 1e3)
    return {k: {"runs_ms": [round(x, 1) for x in v], "best_ms": round(min(v), 1), "spread_ms": round(max(v) - min(v), 1)}
            for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--zeros-mib", type=int, default=256)
    ap.add_argument("--parent-first", action="store_true")
    ap.add_argument("--slabs", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    tile, inline, window = geometry()
    oracle = Oracle()
    maker = FindLib(max_blocks=512)
    text = oracle.synthtext(a.mib << 20, seed=12345)
    z = maker.compress_buffer(text, 9)
    maker.close()
    parent = RangeLib(a.parent_lib, max_blocks=a.slabs) if a.parent_lib and a.parent_first else None
    lib = FindLib(max_blocks=a.slabs)
    if a.parent_lib and not a.parent_first:
        parent = RangeLib(a.parent_lib, max_blocks=a.slabs)
    cap = len(z) // 32 + 64
    at = len(text) // 3
    rare = text[at:at + 16]
    want = FC.hits(text, rare)
    results = {"mib": a.mib, "bz2_bytes": len(z), "slabs": a.slabs, "parent_first": bool(a.parent_first), "rare_hits": len(want), "geometry": [tile, inline, window]}

    rc, hits, total, e, info = lib.find_buffer(z, rare, 1000, cap)
    assert rc == 0 and total == len(want) and hits == want[:1000] and info.out_bytes == len(text), "the hits are not bytes.find's"
    common = text.count(b"e ")                                           # ("e " cannot overlap itself)
    rc, hits, total, _, _ = lib.find_buffer(z, b"e ", 0, cap)
    assert rc == 0 and total == common and hits == []
    results["common_hits"] = common
    sides = {}
    if parent:
        sides["parent_off"] = lambda: parent.index_build(z, cap)
    sides["off"] = lambda: lib.index_build(z, cap)
    sides["rare"] = lambda: lib.find_buffer(z, rare, 1000, cap)
    sides["common"] = lambda: lib.find_buffer(z, b"e ", 0, cap)
    results["text"] = alternate(sides, a.reps)
    results["blocks"] = int(info.nblk)
    for k, v in results["text"].items():
        print(f"text {a.mib} MiB, {info.nblk} blocks, {k}: best {v['best_ms']} ms, spread {v['spread_ms']} ms, runs {v['runs_ms']}", flush=True)

    N = a.zeros_mib << 20
    zz = bz2.compress(bytes(N), 9)
    zcap = len(zz) // 32 + 64
    rc, hits, total, _, info = lib.find_buffer(zz, bytes(4), 5, zcap)
    assert rc == 0 and total == N - 3 and hits == [0, 1, 2, 3, 4] and info.out_bytes == N
    sides = {"off": lambda: lib.index_build(zz, zcap),
             "every4": lambda: lib.find_buffer(zz, bytes(4), 0, zcap),
             "every16": lambda: lib.find_buffer(zz, bytes(16), 0, zcap),
             "every4_list": lambda: lib.find_buffer(zz, bytes(4), 4 * window, zcap)}
    results["zeros_mib"] = a.zeros_mib
    results["zeros"] = alternate(sides, a.reps)
    for k, v in results["zeros"].items():
        print(f"zeros {a.zeros_mib} MiB, {info.nblk} blocks, {k}: best {v['best_ms']} ms, spread {v['spread_ms']} ms, runs {v['runs_ms']}", flush=True)
    print(json.dumps(results))
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
