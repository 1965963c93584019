"""Ad-hoc GPU probe: phase timers of the split kernel (diagnostic build, BZX_LIB=.../libbzx_diag.so) over 1,194 copies of
one text block, ms per block; slot 100 is form_buckets (the greedy walk) and bucket_setup."""
import sys, ctypes as C
sys.path.insert(0, "tests")
from bzx_ctypes import *
o = Oracle(); lib = BzxLib()
L = lib.lib
L.bzx_dbg_time_stages.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_int, C.POINTER(C.c_float)]
L.bzx_dbg_phase_timers.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
reps = 1194
blk = o.synthtext(899981)
ms = (C.c_float * 4)(); t = (C.c_ulonglong * 128)()
lib._check(L.bzx_dbg_time_stages(lib.ctx, blk, len(blk), reps, 1, ms))
lib._check(L.bzx_dbg_phase_timers(lib.ctx, 1, None))
lib._check(L.bzx_dbg_time_stages(lib.ctx, blk, len(blk), reps, 1, ms))
lib._check(L.bzx_dbg_phase_timers(lib.ctx, 0, t))
SPLIT = {96: "fetch", 97: "in-use", 98: "pack", 99: "hist", 100: "form buckets (walk)", 101: "partition", 102: "emit", 103: "deeper"}
print(f"bwt stage {ms[0]:.2f} ms for {reps} copies of one 899,981-byte text block (diagnostic build); split kernel, lane 0's clock, ms per block:")
for k, v in SPLIT.items():
    print(f"  {v:22s} {t[k] / 100e3 / reps:8.4f}")
print(f"  total                  {sum(t[k] for k in SPLIT) / 100e3 / reps:8.4f}")
