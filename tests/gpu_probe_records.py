"""Probe (not a test): what counting records costs the index pass, and what a line-addressed read costs.

  python tests/gpu_probe_records.py [--reps 3] [--mib 256] [--queries 4096] [--parent-lib PATH] [--delim 10]

One input: --mib MiB of seeded synthetic text compressed at -9 by the library.  Index sides, alternated in one process
after a warm-up of every side, best of --reps, host clock around calls that end in a device synchronisation:
bzx_index_build_buffer of another build of the library (--parent-lib: the parent commit's), the same call of this build,
and bzx_index_build_records_buffer.  Then, once each: one bzx_records_locate_buffer of --queries random line numbers, one
bzx_decompress_records_buffer of as many single lines, and a loop of bzx_decompress_range_buffer over the same byte ranges
as the yardstick (all three over the pieces bzx_records_pieces names, read from the file image in memory).  Checked on the
way: the table against numpy, the located offsets and the lines against the text.  When the text holds fewer than 4 x
--queries of the delimiter the probe switches to the space character and says so.  Prints one line per part and a JSON
line."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import records_cases as RC  # noqa: E402
from bzx_ctypes import Oracle  # noqa: E402
from bzx_range_ctypes import RangeLib  # noqa: E402
from bzx_records_ctypes import RecordsLib  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--delim", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.init()
    oracle = Oracle()
    maker = RecordsLib(max_blocks=512)
    lib = RecordsLib(max_blocks=16)
    parent = RangeLib(a.parent_lib, max_blocks=16) if a.parent_lib else None
    text = oracle.synthtext(a.mib << 20, seed=12345)
    z = maker.compress_buffer(text, 9)
    maker.close()
    delim = a.delim
    pos = RC.positions(text, delim)
    if len(pos) < 4 * a.queries:
        print(f"the text holds {len(pos)} bytes {delim}: counting spaces instead", flush=True)
        delim = 0x20
        pos = RC.positions(text, delim)
    cap = len(z) // 32 + 64
    results = {"mib": a.mib, "bz2_bytes": len(z), "delim": delim, "records": int(len(pos))}

    # ---- the index pass
    sides = {"this_off": lambda: lib.index_build(z, cap), "this_on": lambda: lib.index_records(z, delim, cap)}
    if parent:
        sides["parent_off"] = lambda: parent.index_build(z, cap)
    for fn in sides.values():                                           # warm-up and checks
        assert fn()[0] == 0
    rc, e, info, table = lib.index_records(z, delim, cap)
    n = info.nblk
    assert table == RC.table_of(pos, [e[k].out_off for k in range(n)]), "the table is not numpy's"
    t = {k: [] for k in sides}
    for _ in range(a.reps):                                             # sides alternated
        for k, fn in sides.items():
            t[k].append(clock(fn)[0])
    results["index_ms"] = {k: [round(x * 1e3, 1) for x in v] for k, v in t.items()}
    results["blocks"] = n
    print(f"index of {a.mib} MiB, {n} blocks: " + "  ".join(f"{k} best {min(v) * 1e3:.1f} ms (runs {[round(x * 1e3, 1) for x in v]})"
                                                              for k, v in t.items()), flush=True)

    # ---- locate, read, and the loop of single range reads
    rnd = random.Random(4)
    T = len(pos)
    lines = [rnd.randrange(0, T) for _ in range(a.queries)]
    ranges = [(r, 1) for r in lines]
    rc, pieces, np_ = lib.pieces(e, n, table, ranges, cap=n + 2)
    assert rc == 0
    bufs, pc, npc = lib._pieces(z, pieces)
    results["pieces"] = len(pieces)
    results["piece_bytes"] = sum(ln for _, ln in pieces)
    for label in ("first", "second"):
        dt, (rc, offs, st) = clock(lambda: lib.locate_raw(lib.lib.bzx_records_locate_buffer, pc, npc, e, n, table, delim, lines))
        assert rc == 0 and offs == [RC.rec_start(pos, len(text), r) for r in lines]
        results[f"locate_ms_{label}"] = round(dt * 1e3, 1)
    want = [text[RC.rec_start(pos, len(text), r):RC.rec_start(pos, len(text), r + 1)] for r in lines]
    need = sum(map(len, want))
    out = C.create_string_buffer(need + 1)
    for label in ("first", "second"):
        dt, r = clock(lambda: lib.records_raw(lib.lib.bzx_decompress_records_buffer, pc, npc, e, n, table, delim, ranges,
                                              C.addressof(out), need))
        assert r.rc == 0 and r.need == need and out.raw[:need] == b"".join(want)
        results[f"records_ms_{label}"] = round(dt * 1e3, 1)
    st = lib.stats()
    results["distinct_blocks"] = st.nblk

    def loop():
        got = C.c_size_t()
        one = C.create_string_buffer(1 << 20)
        for r, w in zip(lines, want):
            off = RC.rec_start(pos, len(text), r)
            assert lib.lib.bzx_decompress_range_buffer(lib.ctx, z, len(z), 0, e, n, off, len(w), one, C.byref(got)) == 0
            assert got.value == len(w)
    dt, _ = clock(loop)
    results["range_loop_ms"] = round(dt * 1e3, 1)
    print(f"{a.queries} random lines of {T}: locate {results['locate_ms_second']} ms, records read {results['records_ms_second']} ms "
          f"({need} bytes, {st.nblk} distinct blocks, {len(pieces)} pieces of {results['piece_bytes']} bytes), "
          f"loop of bzx_decompress_range_buffer {results['range_loop_ms']} ms", flush=True)
    print(json.dumps(results))
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
