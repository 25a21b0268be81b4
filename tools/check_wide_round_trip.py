"""Manual check (GPU box): round trip of an input beyond 2^32 through the n > 2^32 forward and inverse with no knobs -- the inverse
takes the compact form where the full one does not fit (above ~16 GiB).  Forward, release_memory(), inverse, then a check against the
input regenerated from its seed.  With --pinned the input, the transform and the output live in pinned host blocks (bwts_host_alloc)
and the check runs on the host, a GiB at a time; otherwise all three are device buffers and the check is device_equal.
--inverse-only (with --pinned) skips the forward, for sizes whose forward does not fit: every byte string is a transform, so the
generated input itself is inverted, and the output is checked for what any inverse satisfies -- the same bytes (histograms), and
out[n-1] = in[0] (bwts[0] = T[n-1]) -- plus a factor count of at least one.
    python tools/check_wide_round_trip.py [gib] [kind] [--pinned [--inverse-only]]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as ge
import oracle_lib as O
args = [a for a in sys.argv[1:] if not a.startswith("--")]
pinned = "--pinned" in sys.argv
gib = float(args[0]) if args else 24
kind = args[1] if len(args) > 1 else "dna"
n, seed = int(gib * (1 << 30)), 1
pkg = ge.load_package()
ctx = pkg.Context(0)
res = {"gib": gib, "kind": kind, "n": n, "pinned": pinned}
if pinned:
    hx, x = ctx.host_alloc(n)
    hy, y = ctx.host_alloc(n)
    out = x                                      # the inverse writes over the input: the check regenerates it on the host
else:
    x, y = ctx.alloc(n), ctx.alloc(n)
if "--inverse-only" in sys.argv:
    assert pinned, "--inverse-only keeps its buffers in pinned host memory"
    res["inverse_only"] = True
    ctx.generate(kind, seed, n, y)
    ctx.release_memory()
    t0 = time.perf_counter()
    try:
        ctx.inverse_device(y, n, x)
    except pkg.BwtsError as e:
        res["inverse_error"] = str(e)
        print(json.dumps(res)); print("FAILED"); sys.exit(1)
    res["inverse_s"] = time.perf_counter() - t0
    t = ctx.timings()
    res.update(inverse_device_ms=t.total_ms, inverse_device_bytes=t.device_bytes, inverse_bytes_per_n=t.device_bytes / n, factors=t.factors)
    print("inverse %.1f s (%.0f ms device), device_bytes %.1f GiB = %.2f n" % (res["inverse_s"], t.total_ms, t.device_bytes / 2**30, t.device_bytes / n), flush=True)
    hi, ho = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for o in range(0, n, 1 << 30):
        hi += np.bincount(hy[o:o + (1 << 30)], minlength=256); ho += np.bincount(hx[o:o + (1 << 30)], minlength=256)
    res.update(histograms_equal=bool(np.array_equal(hi, ho)), last_is_first=bool(hx[n - 1] == hy[0]))
    res["round_trip_ok"] = res["histograms_equal"] and res["last_is_first"] and t.factors >= 1
    print(json.dumps(res)); print("OK" if res["round_trip_ok"] else "FAILED")
    ctx.close()
    sys.exit(0 if res["round_trip_ok"] else 1)
ctx.generate(kind, seed, n, x)
t0 = time.perf_counter(); ctx.forward_device(x, n, y); res["forward_s"] = time.perf_counter() - t0
t = ctx.timings(); res["forward_device_bytes"] = t.device_bytes; fwd_factors = t.factors
print("forward %.1f s, device_bytes %.1f GiB" % (res["forward_s"], t.device_bytes / 2**30), flush=True)
if not pinned:
    x.free()
ctx.release_memory()
if not pinned:
    out = ctx.alloc(n)
t0 = time.perf_counter()
try:
    ctx.inverse_device(y, n, out)
except pkg.BwtsError as e:
    res["inverse_error"] = str(e)
    print(json.dumps(res)); print("FAILED"); sys.exit(1)
res["inverse_s"] = time.perf_counter() - t0
t = ctx.timings()
res.update(inverse_device_ms=t.total_ms, inverse_device_bytes=t.device_bytes, inverse_bytes_per_n=t.device_bytes / n,
           factors=t.factors, factors_equal=t.factors == fwd_factors)
print("inverse %.1f s (%.0f ms device), device_bytes %.1f GiB = %.2f n" % (res["inverse_s"], t.total_ms, t.device_bytes / 2**30, t.device_bytes / n), flush=True)
if pinned:
    ok = True
    for o in range(0, n, 1 << 30):
        c = min(1 << 30, n - o)
        if not np.array_equal(hx[o:o + c], O.generate(kind, c, seed, off=o)):
            ok = False; break
else:
    y.free()
    x = ctx.alloc(n)
    ctx.generate(kind, seed, n, x)
    ok = ctx.device_equal(x, out, n)
res["round_trip_ok"] = bool(ok) and res["factors_equal"]
print(json.dumps(res))
print("OK" if res["round_trip_ok"] else "FAILED")
ctx.close()
sys.exit(0 if res["round_trip_ok"] else 1)
