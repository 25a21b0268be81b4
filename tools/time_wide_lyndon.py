"""Manual measurement (GPU box): the forward of n = 2^32 + 2^28 bytes of Lyndon blocks (tests/lyndon_blocks.py: zero runs of 65..123
bytes before 200..2000 random non-zero bytes, millions of factor candidates), which takes the suffix route to the Lyndon factors
(wide_path.h).  BWTS_ROUND_TRACE=1 makes the engine print the route's own wall time; timing level 2 gives every kernel class of the
whole call.  Two calls: the first takes the arenas, the second finds them in place.
    python tools/time_wide_lyndon.py [log2n_extra]      (n = 2^32 + 2^log2n_extra, default 28)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["BWTS_ROUND_TRACE"] = "1"
import numpy as np
import lyndon_blocks as LB
import __graft_entry__ as ge
pkg = ge.load_package()
extra = int(sys.argv[1]) if len(sys.argv) > 1 else 28
t0 = time.perf_counter()
x, starts = LB.big_lyndon_blocks((1 << 32) + (1 << extra))
n, k = x.size, starts.size
print("input: n %d, %d blocks, %d zeros, built in %.0f s" % (n, k, int(np.count_nonzero(x == 0)), time.perf_counter() - t0), flush=True)
ctx = pkg.Context(0)
ctx.set_timing(2)
a, b = ctx.alloc(n), ctx.alloc(n)
a.upload(x)
del x, starts
for call in range(2):
    t0 = time.perf_counter()
    ctx.forward_device(a, n, b)
    dt = time.perf_counter() - t0
    t = ctx.timings().as_dict()
    print("call %d: %.0f ms wall, device %.0f ms, factors %d (blocks %d), suffix rounds %d, rounds %d, tied %d, device GiB %.1f" %
          (call, 1e3 * dt, t["total_ms"], t["factors"], k, t["lyndon_rounds"], t["rounds"], t["active_after_round0"], t["device_bytes"] / 2**30),
          flush=True)
    print("   kernel classes (ms):", {c: round(v["ms"], 1) for c, v in t["kernels"].items() if v["ms"] > 0}, flush=True)
a.free(); b.free(); ctx.close()
