"""Probe (not a test): what the hits' line numbers cost the index pass, and what grep costs.

  python tests/gpu_probe_grep.py [--reps 3] [--mib 256] [--slabs 256] [--parent-lib PATH] [--common-max-hits N]

Input: --mib MiB of seeded synthetic text compressed at -9 by the library.  Sides, alternated in one process after a
warm-up of every side, host clock around calls that end in a device synchronisation, every run listed with its best
and its spread (max - min):
  parent_find  bzx_find_buffer of another build of the library (--parent-lib: the parent commit's), a rare 16-byte pattern
  find_off     the same call of this build: find on, lines off
  pass_off     begin, bzx_index_find, one feed of the whole input from a buffer made once, end: find on, lines off
  pass_lines   the same with bzx_index_find_lines ('\\n') behind the find: the lines forms of the three kernels
  pass_off_common, pass_lines_common  the two with a pattern of about one hit per line and max_hits = --common-max-hits: the lines of the windows
  grep_rare    bzx_grep_buffer, the rare pattern: the pass with find, lines and the record table, then the record read
  grep_common  bzx_grep_buffer, the common pattern, max_hits = --common-max-hits (the records of the listed hits)
The hits, lines and records of the rare pattern are checked first, against bytes.find, bytes.count and the lines cut
out of the text (the rule of tests/grep_cases.py, without its tables).
Prints one line per side and a JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import find_cases as FC  # noqa: E402
from bzx_ctypes import Oracle  # noqa: E402
from bzx_find_ctypes import FindLib  # noqa: E402
from bzx_grep_ctypes import GrepLib, geometry  # noqa: E402

NL = 10


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


def one_pass(lib, zbuf, n, pat, max_hits, delim):
    """begin, find, (lines), one final feed of the whole input, end -> (rc, total hits, lines listed)"""
    L = lib.lib
    h = C.c_void_p()
    assert L.bzx_index_begin(lib.ctx, min(n, 64 << 20), C.byref(h)) == 0
    try:
        assert L.bzx_index_find(h, pat, len(pat), max_hits) == 0
        if delim is not None:
            assert L.bzx_index_find_lines(h, delim) == 0
        pos, done, rc = 0, 0, 0
        while not rc and not (done and pos == n):
            used, d = C.c_size_t(0), C.c_int(0)
            rc = L.bzx_index_feed(h, C.addressof(zbuf) + pos, n - pos, 1, C.byref(used), C.byref(d))
            pos += used.value
            done = d.value
        hp, nl, total = C.POINTER(C.c_uint64)(), C.c_uint64(), C.c_uint64()
        assert L.bzx_index_get_hits(h, C.byref(hp), C.byref(nl), C.byref(total)) == 0
        nlines = 0
        if delim is not None:
            lp, n2 = C.POINTER(C.c_uint64)(), C.c_uint64()
            assert L.bzx_index_get_hit_lines(h, C.byref(lp), C.byref(n2)) == 0 and n2.value == nl.value
            nlines = n2.value
        return rc, total.value, nlines
    finally:
        L.bzx_index_end(h)


def model(text, hit_list):
    """grep_cases.lines_of and grep_cases.grep for a text too long for their tables: one walk over the text.
    -> ([line of every hit], [distinct lines], [their records])"""
    lines, prev, acc = [], 0, 0
    for p in hit_list:
        acc += text.count(b"\n", prev, p)
        prev = p
        lines.append(acc)
    nums, recs = [], []
    for p, ln in zip(hit_list, lines):
        if nums and nums[-1] == ln:
            continue
        end = text.find(b"\n", p)
        nums.append(ln)
        recs.append(text[text.rfind(b"\n", 0, p) + 1:end + 1 if end >= 0 else len(text)])
    return lines, nums, recs


class GrepCall:
    """bzx_grep_buffer into buffers made once."""

    def __init__(self, lib, z, cap_recs, cap):
        self.lib, self.z, self.cap_recs, self.cap = lib, z, cap_recs, cap
        self.recs = (C.c_uint64 * cap_recs)()
        self.offs, self.lens = (C.c_size_t * cap_recs)(), (C.c_size_t * cap_recs)()
        self.out = C.create_string_buffer(cap)
        self.nrecs, self.need, self.total, self.trunc = C.c_uint64(), C.c_size_t(), C.c_uint64(), C.c_int()

    def __call__(self, pat, max_hits):
        rc = self.lib.lib.bzx_grep_buffer(self.lib.ctx, self.z, len(self.z), pat, len(pat), NL, max_hits, self.recs, self.cap_recs,
                                          C.byref(self.nrecs), self.out, self.cap, self.offs, self.lens, C.byref(self.need),
                                          C.byref(self.total), C.byref(self.trunc))
        return rc, self.nrecs.value, self.need.value, self.total.value, self.trunc.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--slabs", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--common-max-hits", type=int, default=1_000_000)
    a = ap.parse_args()
    torch.cuda.init()
    tile, inline, window = geometry()
    oracle = Oracle()
    maker = FindLib(max_blocks=512)
    text = oracle.synthtext(a.mib << 20, seed=12345)
    z = maker.compress_buffer(text, 9)
    maker.close()
    lib = GrepLib(max_blocks=a.slabs)
    parent = FindLib(a.parent_lib, max_blocks=a.slabs) if a.parent_lib else None
    cap = len(z) // 32 + 64
    zbuf = C.create_string_buffer(z, len(z))
    nlines = text.count(b"\n")
    at = len(text) // 3
    rare = text[at:at + 16].replace(b"\n", b" ")
    want = FC.hits(text, rare)
    # the pattern whose count comes closest to one per line
    common = min((b"e ", b"th", b". ", b", ", b"the ", b"s "), key=lambda p: abs(text.count(p) - nlines))
    ncommon = text.count(common)
    results = {"mib": a.mib, "bz2_bytes": len(z), "slabs": a.slabs, "lines": nlines, "rare_hits": len(want),
               "common": common.decode(), "common_hits_nonoverlapping": ncommon, "common_max_hits": a.common_max_hits,
               "geometry": [tile, inline, window]}

    # the answers first
    rc, keys, info, hits, total, lrc, lines, _ = lib.index_feed_lines(z, rare, 1000, NL)
    want_lines, nums, recs = model(text, want[:1000])
    assert rc == 0 and lrc == 0 and total == len(want) and hits == want[:1000] and lines == want_lines, "lines differ"
    grep = GrepCall(lib, z, max(a.common_max_hits, 1024), len(text) + 16)
    rc, nrecs, need, total, trunc = grep(rare, 1000)
    assert rc == 0 and nrecs == len(nums) and list(grep.recs[:nrecs]) == nums and need == sum(map(len, recs)), lib.last_error()
    assert grep.out.raw[:need] == b"".join(recs), "records differ"
    rc, nrecs, need, total, trunc = grep(common, a.common_max_hits)
    assert rc == 0, lib.last_error()
    results["grep_common"] = {"records": nrecs, "bytes": need, "total_hits": total, "truncated": trunc}

    sides = {}
    if parent:
        sides["parent_find"] = lambda: parent.find_buffer(z, rare, 1000, cap)
    sides["find_off"] = lambda: lib.find_buffer(z, rare, 1000, cap)
    sides["pass_off"] = lambda: one_pass(lib, zbuf, len(z), rare, 1000, None)
    sides["pass_lines"] = lambda: one_pass(lib, zbuf, len(z), rare, 1000, NL)
    sides["pass_off_common"] = lambda: one_pass(lib, zbuf, len(z), common, a.common_max_hits, None)
    sides["pass_lines_common"] = lambda: one_pass(lib, zbuf, len(z), common, a.common_max_hits, NL)
    sides["grep_rare"] = lambda: grep(rare, 1000)
    sides["grep_common"] = lambda: grep(common, a.common_max_hits)
    results["sides"] = alternate(sides, a.reps)
    results["blocks"] = int(info.nblk)
    for k, v in results["sides"].items():
        print(f"text {a.mib} MiB, {info.nblk} blocks, {k}: best {v['best_ms']} ms, spread {v['spread_ms']} ms, runs {v['runs_ms']}", flush=True)
    print(json.dumps(results))
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
