"""Probe (not a test): what a salvage index costs beside the plain index it equals on a clean input.

  python tests/gpu_probe_salvage.py [--reps 3] [--mib 256] [--parent-lib PATH]

One stream of --mib MiB of seeded synthetic text at -9.  Sides, alternated in one process after a warm-up of every side,
best of --reps: bzx_index_build_buffer of this build, bzx_salvage_build_buffer of the clean stream, the same of a damaged
variant (a payload bit of every 50th block flipped), bzx_salvage_buffer of the damaged variant (salvage index + range read of
everything that survived), and with --parent-lib the same four calls of another build of the library (the parent
commit's).  Times are host clock around calls that end in a device synchronise.  Checked on the way: on the clean stream
the salvage entries are the index's and there is no gap; the damaged variant loses exactly the blocks hit, and its
salvaged bytes are the surviving blocks' bytes.  Prints one line and a JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bzx_ctypes import Oracle  # noqa: E402
from bzx_range_ctypes import RangeLib  # noqa: E402
from bzx_salvage_ctypes import SalvageLib  # noqa: E402

MAX_BLOCKS = 320            # a 256 MiB input at -9 is 299 blocks: one round


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    raw = Oracle().synthtext(a.mib << 20, seed=12345)
    maker = RangeLib(max_blocks=MAX_BLOCKS)
    z = maker.compress_buffer(raw, 9)
    maker.close()
    lib = SalvageLib(max_blocks=MAX_BLOCKS)
    parent = SalvageLib(a.parent_lib, max_blocks=MAX_BLOCKS) if a.parent_lib else None
    cap = len(z) // 2000 + 4096

    rc, e, info = lib.index_build(z, cap=cap)
    assert rc == 0 and info.out_bytes == len(raw), lib.last_error()
    n = info.nblk
    hit = list(range(49, n, 50))
    bad = bytearray(z)
    for k in hit:
        bit = e[k].bit + e[k].img_bits // 2
        bad[bit >> 3] ^= 0x80 >> (bit & 7)
    bad = bytes(bad)
    alive = [k for k in range(n) if k not in hit]
    want = b"".join(raw[e[k].out_off:e[k].out_off + e[k].out_len] for k in alive)

    def sides_of(which, pre):
        return {
            pre + "index": lambda: which.index_build(z, cap=cap),
            pre + "salvage_clean": lambda: which.salvage_build(z, cap=cap, cap_gaps=4096),
            pre + "salvage_damaged": lambda: which.salvage_build(bad, cap=cap, cap_gaps=4096),
            pre + "salvage_buffer_damaged": lambda: which.salvage_buffer(bad, len(want)),
        }

    sides = sides_of(lib, "")
    if parent:
        sides.update(sides_of(parent, "parent_"))
    # warm-up and checks
    rc, e2, inf2, gaps, ng = sides["salvage_clean"]()
    assert rc == 0 and ng == 0 and bytes(e2)[:40 * n] == bytes(e)[:40 * n] and inf2.nblk == n and inf2.nstreams == info.nstreams
    rc, e3, inf3, gaps, ng = sides["salvage_damaged"]()
    assert rc == 0 and inf3.nblk == len(alive) and [e3[i].bit for i in range(inf3.nblk)] == [e[k].bit for k in alive]
    assert ng == len(hit) and [g[0] for g in gaps] == [e[k].bit for k in hit]
    rc, got, out_len, _, _ = sides["salvage_buffer_damaged"]()
    assert rc == 0 and got == want, lib.last_error()
    sides["index"]()
    if parent:
        rc, ep, infp = sides["parent_index"]()
        assert rc == 0 and bytes(ep)[:40 * n] == bytes(e)[:40 * n]
        for k in ("parent_salvage_clean", "parent_salvage_damaged", "parent_salvage_buffer_damaged"):
            assert sides[k]()[0] == 0, parent.last_error()
    t = {k: [] for k in sides}
    for _ in range(a.reps):                                         # sides alternated
        for k, fn in sides.items():
            t[k].append(timed(fn)[0])
    r = {k: round(min(v) * 1e3, 2) for k, v in t.items()}
    print(f"{a.mib} MiB -9, {n} blocks, {len(hit)} hit: " + "  ".join(f"{k} {v} ms" for k, v in r.items()), flush=True)
    r.update(blocks=n, hit=len(hit), bz2_bytes=len(z), all_ms={k: [round(x * 1e3, 2) for x in v] for k, v in t.items()})
    print(json.dumps(r))
    lib.close()
    if parent:
        parent.close()


if __name__ == "__main__":
    main()
