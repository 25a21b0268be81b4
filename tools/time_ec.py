"""Manual timing (GPU box) of the entropy coder beside the move-to-front stage, in one process, all times total_ms of the call:
the bench default zipf(2^30, seed 1) generated on the device and transformed once, every call warmed up, then the four calls
alternated -- mtf_forward_device on the BWTS, ec_encode_device on the ranks, ec_decode_device, mtf_inverse_device -- and the minimum of
--reps rounds each, with the per-launch spans of the two coder calls.  The bar: each direction of the coder costs no more than the MTF
call beside it (ec_encode_ms <= mtf_forward_ms, ec_decode_ms <= mtf_inverse_ms), both sides from this run; exit code 1 when it is
missed.  Beside the times: compressed bytes / n and the order-0 entropy of the ranks.  For the record: uniform256(2^28), which the
coder can only expand, and the segment forms at 16384 x 64 KiB and at segments of 64 KiB + 1 (unaligned starts).
    python tools/time_ec.py [--log2n 30] [--reps 6] > profiles/ec_stage.txt"""
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


def entropy_bits_per_byte(pkg, buf, n):
    """order-0 entropy of n device bytes, from a histogram taken on the host in pieces"""
    h = np.zeros(256, dtype=np.int64)
    piece = 64 << 20
    for at in range(0, n, piece):
        m = min(piece, n - at)
        out = np.empty(m, dtype=np.uint8)
        buf.ctx._check(pkg.lib().bwts_copy_to_host(buf.ctx._h, out.ctypes.data, buf.ptr + at, m))
        h += np.bincount(out, minlength=256)
    p = h[h > 0] / float(n)
    return float(-(p * np.log2(p)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 6)
    pkg = ge.load_package()
    with pkg.Context(0) as ctx:
        cap = pkg.ec_bound_segments(np.full(max(n >> 16, 1), min(n, 1 << 16), dtype=np.uint64))      # (the largest bound used below)
        x, y, r, back = (ctx.alloc(n) for _ in range(4))
        s = ctx.alloc(cap)
        size = {}
        ctx.generate("zipf", 1, n, x)
        ctx.forward_device(x, n, y)
        calls = [("mtf_forward_device", lambda: ctx.mtf_forward_device(y, n, r)),
                 ("ec_encode_device", lambda: size.update(one=ctx.ec_encode_device(r, n, s, cap))),
                 ("ec_decode_device", lambda: ctx.ec_decode_device(s, size["one"], back, n)),
                 ("mtf_inverse_device", lambda: ctx.mtf_inverse_device(r, n, back))]
        rounds(ctx, calls, 1)                                    # warm-up: arenas, code object, every kernel once
        ctx.ec_decode_device(s, size["one"], back, n)
        assert ctx.device_equal(back, r, n), "ec_decode(ec_encode(ranks)) != ranks"
        print("zipf 2^%d, seed 1 (the bench default): %d rounds, the four calls alternated" % (args.log2n, reps))
        m = report(rounds(ctx, calls, reps))
        ok_e, ok_d = m["ec_encode_device"] <= m["mtf_forward_device"], m["ec_decode_device"] <= m["mtf_inverse_device"]
        print("  bar: ec_encode_ms <= mtf_forward_ms: %s (%.3f vs %.3f); ec_decode_ms <= mtf_inverse_ms: %s (%.3f vs %.3f)" % (
            "holds" if ok_e else "MISSED", m["ec_encode_device"], m["mtf_forward_device"], "holds" if ok_d else "MISSED",
            m["ec_decode_device"], m["mtf_inverse_device"]), flush=True)
        ent = entropy_bits_per_byte(pkg, r, n)
        print("  compressed %d bytes / n = %.4f; order-0 entropy of the ranks %.4f bits per byte = %.4f of n" % (
            size["one"], size["one"] / n, ent, ent / 8), flush=True)
        ctx.set_timing(2)
        launches = {"ec_encode_device": ["block histograms", "normalise", "count pass", "size scan", "encode pass"],
                    "ec_decode_device": ["directory gather", "size scan", "decode"]}
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
        calls = [("ec_encode_device", lambda: size.update(uni=ctx.ec_encode_device(x, m2, s, cap))),
                 ("ec_decode_device", lambda: ctx.ec_decode_device(s, size["uni"], back, m2))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, x, m2)
        print("uniform256 2^%d (every step emits: the expansion path; for the record): compressed / n = %.4f" % (int(np.log2(m2)), size["uni"] / m2))
        report(rounds(ctx, calls, reps))

        seg = min(n, 64 << 10)
        ls = np.full(n // seg, seg, dtype=np.uint64)
        ctx.generate("zipf", 1, n, x)
        ctx.forward_segments_device(x, ls, y)
        ctx.mtf_forward_segments_device(y, ls, r)
        calls = [("ec_encode_segments_device", lambda: size.update(seg=ctx.ec_encode_segments_device(r, ls, s, cap))),
                 ("ec_decode_segments_device", lambda: ctx.ec_decode_segments_device(s, size["seg"], ls, back))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, r, n)
        print("zipf 2^%d in %d segments of 64 KiB, ranks of the segmented BWTS (no bar): compressed / n = %.4f" % (
            args.log2n, ls.size, float(size["seg"].sum()) / n))
        report(rounds(ctx, calls, reps))

        seg = min(n, (64 << 10) + 1)
        ls = np.full(n // seg, seg, dtype=np.uint64)
        m3 = int(ls.sum())
        calls = [("ec_encode_segments_device", lambda: size.update(odd=ctx.ec_encode_segments_device(r, ls, s, cap))),
                 ("ec_decode_segments_device", lambda: ctx.ec_decode_segments_device(s, size["odd"], ls, back))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, r, m3)
        print("the same ranks cut into %d segments of 64 KiB + 1: all but the first start off a 16-byte boundary, the byte side goes through "
              "single-byte loads and stores (no bar)" % ls.size)
        report(rounds(ctx, calls, reps))
        for d in (x, y, r, back, s):
            d.free()
    return 0 if ok_e and ok_d else 1


if __name__ == "__main__":
    sys.exit(main())
