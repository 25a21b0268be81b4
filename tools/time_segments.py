"""Manual timing (GPU box): 1 GiB of zipf and of text cut into 4 KiB, 64 KiB, 256 KiB and 1 MiB segments, through
bwts_forward_segments_device / bwts_inverse_segments_device, against the same segments through one forward_device / inverse_device
call each (a 4096-segment sample where there are more, scaled up) and through bwts_forward_batch, and against the whole 1 GiB as one
input; then two skewed segmentations ([n/4, 1] and [100000, 100000]) against one call per segment.  Wall time (timing off) and device time (total_ms), then
a level-2 kernel table of one segmented forward and inverse.
    python tools/time_segments.py [--log2n 30] > profiles/segments_<date>.txt
--inverse-only: the segmented inverse alone, one row per set -- 4 KiB, 64 KiB, 256 KiB, 1 MiB and 16 MiB segments, the mixed 4 KiB .. 1 MiB
set and [100000, 100000] -- with the plan the call took (Context.debug_segments_report), every repeat listed, and a level-2 kernel table at
1 MiB segments.  BWTS_TEST_KNOBS=1 BWTS_SEG_INV_PLAN=lane|shared in the environment forces the plan.
    python tools/time_segments.py --inverse-only > profiles/segments_inverse_<date>.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def best(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts)


def kernel_table(pkg, ctx, title):
    t = ctx.timings()
    print("  %s: total %.2f ms, factors/cycles %d, rounds %d" % (title, t.total_ms, t.factors, t.rounds))
    for k in range(pkg.K_COUNT):
        if t.k[k].launches:
            print("    %-22s %9.3f ms  %6d launches" % (pkg.lib().bwts_kernel_class_name(k).decode(), t.k[k].ms, t.k[k].launches))


def mixed_lengths(n):
    """Power-of-two lengths from 4 KiB to 1 MiB at random, until n bytes (the set of tests/test_segments.py::test_segments_1gib_mixed)."""
    rng = np.random.default_rng(9)
    ls, left = [], n
    while left:
        m = int(min(left, 1 << int(rng.integers(12, 21))))
        ls.append(m)
        left -= m
    return np.array(ls, dtype=np.uint64)


def inverse_only(pkg, args, n):
    with pkg.Context(0) as ctx:
        a, b, c = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        for kind in ("zipf", "text"):
            ctx.generate(kind, 1, n, a)
            ctx.forward_device(a, n, b)
            ctx.inverse_device(b, n, c)
            print("%s 2^%d whole input: inverse %.2f ms" % (kind, args.log2n, best(lambda: ctx.inverse_device(b, n, c), args.reps)), flush=True)
            sets = [("%d x %d KiB" % (n >> lg, 1 << (lg - 10)), np.full(n >> lg, 1 << lg, dtype=np.uint64)) for lg in (12, 16, 18, 20, 24) if lg < args.log2n]
            sets += [("mixed 4 KiB .. 1 MiB", mixed_lengths(n)), ("[100000, 100000]", np.array([100000, 100000], dtype=np.uint64))]
            for name, ls in sets:
                m = int(ls.sum())
                ctx.forward_segments_device(a, ls, b)
                ctx.inverse_segments_device(b, ls, c)
                assert ctx.device_equal(a, c, m)
                ts = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    ctx.inverse_segments_device(b, ls, c)
                    ts.append(1e3 * (time.perf_counter() - t0))
                ctx.set_timing(2)
                ctx.inverse_segments_device(b, ls, c)
                tk = ctx.timings().as_dict()["kernels"]
                ctx.set_timing(0)
                rep = ctx.debug_segments_report() if hasattr(ctx, "debug_segments_report") else {}
                how = "plan %s, big %d, %d run(s), %d single" % (rep["plan"], rep["big"], rep["runs"], rep["single_segments"]) if rep else "lane walk or single calls"
                print("  %s %s (%d segments): inverse %.2f ms (repeats %s; timed: lf_build %.2f, walk %.2f ms), attempts %d; %s" % (
                    kind, name, ls.size, min(ts), " ".join("%.2f" % t for t in ts), tk.get("lf_build", {}).get("ms", 0.0), tk.get("walk", {}).get("ms", 0.0),
                    ctx.timings().attempts, how), flush=True)
            if args.log2n > 20:
                ls = np.full(n >> 20, 1 << 20, dtype=np.uint64)
                ctx.forward_segments_device(a, ls, b)
                ctx.set_timing(2)
                ctx.inverse_segments_device(b, ls, c)
                kernel_table(pkg, ctx, "%s 1 MiB segments, inverse" % kind)
                ctx.set_timing(0)
        for d in (a, b, c):
            d.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inverse-only", action="store_true")
    args = ap.parse_args()
    n = 1 << args.log2n
    pkg = ge.load_package()
    if args.inverse_only:
        return inverse_only(pkg, args, n)
    with pkg.Context(0) as ctx:
        a, b, c, d_tmp = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
        for kind in ("zipf", "text"):
            ctx.generate(kind, 1, n, a)
            ctx.forward_device(a, n, b)
            whole_f = best(lambda: ctx.forward_device(a, n, b), args.reps)
            whole_fd = ctx.timings().total_ms
            ctx.inverse_device(b, n, c)
            whole_i = best(lambda: ctx.inverse_device(b, n, c), args.reps)
            print("%s 2^%d whole input: forward %.2f ms (device %.2f), inverse %.2f ms" % (kind, args.log2n, whole_f, whole_fd, whole_i), flush=True)
            for seg_log2 in (12, 16, 18, 20):
                seg = 1 << seg_log2
                count = n // seg
                ls = np.full(count, seg, dtype=np.uint64)
                ctx.forward_segments_device(a, ls, b)
                f = best(lambda: ctx.forward_segments_device(a, ls, b), args.reps)
                fd = ctx.timings().total_ms
                ctx.inverse_segments_device(b, ls, c)
                inv = best(lambda: ctx.inverse_segments_device(b, ls, c), args.reps)
                idev = ctx.timings().total_ms
                assert ctx.device_equal(a, c, n)
                # the same segments one call each (a 4096-segment sample at 4 KiB, scaled up), and through forward_batch
                sample = min(count, 4096)
                scale = count / sample
                note = " (scaled from %d)" % sample if scale > 1 else ""

                def per_call_f():
                    for s in range(sample):
                        ctx.forward_device(a.ptr + s * seg, seg, d_tmp.ptr + s * seg)

                def per_call_i():
                    for s in range(sample):
                        ctx.inverse_device(b.ptr + s * seg, seg, d_tmp.ptr + s * seg)
                pcf = best(per_call_f, 1) * scale
                pci = best(per_call_i, 1) * scale
                x = a.download(sample * seg)
                items = [x[s * seg:(s + 1) * seg] for s in range(sample)]
                bt = best(lambda: ctx.forward_batch(items), 1) * scale
                print("  %s x %d KiB (%d segments): forward %.2f ms (device %.2f), one call each %.0f ms%s, forward_batch %.0f ms: %.1fx, "
                      "%.2fx the whole input; inverse %.2f ms (device %.2f), one call each %.0f ms%s: %.1fx" % (
                          kind, seg >> 10, count, f, fd, pcf, note, bt, pcf / f, f / whole_f, inv, idev, pci, note, pci / inv), flush=True)
            # skewed: one long segment and a one-byte one; two mid-size segments
            for ls in (np.array([(n >> 2), 1], dtype=np.uint64), np.array([100000, 100000], dtype=np.uint64)):
                m = int(ls.sum())
                ctx.forward_segments_device(a, ls, b)
                f = best(lambda: ctx.forward_segments_device(a, ls, b), args.reps)
                inv = best(lambda: ctx.inverse_segments_device(b, ls, c), args.reps)
                assert ctx.device_equal(a, c, m)
                off = np.concatenate([[0], np.cumsum(ls)]).astype(np.int64)

                def calls_f():
                    for s in range(ls.size):
                        ctx.forward_device(a.ptr + int(off[s]), int(ls[s]), d_tmp.ptr + int(off[s]))

                def calls_i():
                    for s in range(ls.size):
                        ctx.inverse_device(b.ptr + int(off[s]), int(ls[s]), d_tmp.ptr + int(off[s]))
                print("  %s segments %s: forward %.2f ms, one call each %.2f ms; inverse %.2f ms, one call each %.2f ms" % (
                    kind, list(map(int, ls)), f, best(calls_f, args.reps), inv, best(calls_i, args.reps)), flush=True)
            ls = np.full(n >> 16, 1 << 16, dtype=np.uint64)
            ctx.set_timing(2)
            ctx.forward_segments_device(a, ls, b)
            kernel_table(pkg, ctx, "%s 64 KiB segments, forward" % kind)
            ctx.inverse_segments_device(b, ls, c)
            kernel_table(pkg, ctx, "%s 64 KiB segments, inverse" % kind)
            ctx.set_timing(0)
        for d in (a, b, c, d_tmp):
            d.free()


if __name__ == "__main__":
    main()
