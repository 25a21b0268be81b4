"""Manual timing (GPU box) of the move-to-front stage beside the transform, in one process, all times total_ms of the call:
the bench default zipf(2^30, seed 1) generated on the device, every call warmed up, then the four calls alternated -- forward_device,
mtf_forward_device on its output, mtf_inverse_device, inverse_device -- and the minimum of --reps rounds each.  The bar: the stage
costs no more than the transform it sits beside (mtf_forward_ms <= forward_ms, mtf_inverse_ms <= inverse_ms), both sides from this
run.  For the record: the two MTF times on uniform256(2^28), which has no runs and shows the in-tile kernel's bare rate, and the
segment forms at 16384 x 64 KiB.
    python tools/time_mtf.py [--log2n 30] [--reps 6] > profiles/mtf_stage.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def rounds(ctx, calls, reps):
    """calls: [(name, fn)]; every round runs them in order; -> {name: [total_ms per round]}"""
    ts = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            fn()
            ts[name].append(ctx.timings().total_ms)
    return ts


def report(ts):
    for name, v in ts.items():
        print("  %-28s min %8.3f ms   (%s)" % (name, min(v), " ".join("%.3f" % x for x in v)), flush=True)
    return {name: min(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    args = ap.parse_args()
    n = 1 << args.log2n
    pkg = ge.load_package()
    with pkg.Context(0) as ctx:
        x, y, r, back = (ctx.alloc(n) for _ in range(4))
        ctx.generate("zipf", 1, n, x)
        calls = [("forward_device", lambda: ctx.forward_device(x, n, y)), ("mtf_forward_device", lambda: ctx.mtf_forward_device(y, n, r)),
                 ("mtf_inverse_device", lambda: ctx.mtf_inverse_device(r, n, back)), ("inverse_device", lambda: ctx.inverse_device(y, n, back))]
        rounds(ctx, calls, 1)                                    # warm-up: arenas, code object, every kernel once
        ctx.mtf_inverse_device(r, n, back)
        assert ctx.device_equal(back, y, n), "mtf_inverse(mtf_forward(bwts)) != bwts"
        print("zipf 2^%d, seed 1 (the bench default): %d rounds, the four calls alternated" % (args.log2n, args.reps))
        m = report(rounds(ctx, calls, max(args.reps, 6)))
        ok_f, ok_i = m["mtf_forward_device"] <= m["forward_device"], m["mtf_inverse_device"] <= m["inverse_device"]
        print("  bar: mtf_forward_ms <= forward_ms: %s (%.3f vs %.3f); mtf_inverse_ms <= inverse_ms: %s (%.3f vs %.3f)" % (
            "holds" if ok_f else "MISSED", m["mtf_forward_device"], m["forward_device"], "holds" if ok_i else "MISSED",
            m["mtf_inverse_device"], m["inverse_device"]), flush=True)
        ctx.set_timing(2)
        launches = {"mtf_forward_device": ["tile states", "group reduce", "top scan", "prefix write", "in-tile"],
                    "mtf_inverse_device": ["in-tile", "group reduce", "top scan", "prefix write", "remap"]}
        for name, fn in calls[1:3]:
            fn()
            t = ctx.timings()
            other = t.as_dict()["kernels"]["other"]
            print("  %s with per-kernel events: total %.3f ms, class other %.3f ms in %d launches: %s" % (
                name, t.total_ms, other["ms"], other["launches"],
                ", ".join("%s %.3f" % (k, ms) for k, ms in zip(launches[name], ctx.debug_last_spans()))))
        ctx.set_timing(0)

        m2 = min(n, 1 << 28)
        ctx.generate("uniform256", 1, m2, x)
        calls = [("mtf_forward_device", lambda: ctx.mtf_forward_device(x, m2, r)), ("mtf_inverse_device", lambda: ctx.mtf_inverse_device(r, m2, back))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, x, m2)
        print("uniform256 2^%d (no runs: the in-tile kernel's bare rate; for the record)" % int(np.log2(m2)))
        report(rounds(ctx, calls, max(args.reps, 6)))

        seg = 64 << 10
        ls = np.full(n // seg, seg, dtype=np.uint64)
        ctx.generate("zipf", 1, n, x)
        ctx.forward_segments_device(x, ls, y)
        calls = [("mtf_forward_segments_device", lambda: ctx.mtf_forward_segments_device(y, ls, r)),
                 ("mtf_inverse_segments_device", lambda: ctx.mtf_inverse_segments_device(r, ls, back))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, y, n)
        print("zipf 2^%d in %d segments of 64 KiB, MTF of the segmented BWTS (no bar)" % (args.log2n, ls.size))
        report(rounds(ctx, calls, max(args.reps, 6)))
        for d in (x, y, r, back):
            d.free()
    return 0 if ok_f and ok_i else 1


if __name__ == "__main__":
    sys.exit(main())
