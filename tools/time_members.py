"""Manual timing (GPU box) of the member frame (include/bwts_members.h) and of the split at a width per segment, in one process, all
times total_ms of the call: zipf(seed 1) generated on the device, every call warmed up, then the calls alternated and the minimum of
--reps rounds each.  No bars: the figures are for the record.
  (a) split and join of 2^log2n bytes as segments of 64 KiB: bwts_planes_*_segments_w_device with every width 4 beside the uniform
      bwts_planes_*_segments_device at width 4 (the kernel that was there before, the yardstick); with the widths cycling 1, 2, 4, 8
      beside a plain device copy (copy_pieces_kernel, one piece) and beside one uniform launch per width class over a quarter of the
      segments each (what launching per class would cost, were the classes contiguous);
  (b) bwts_pack_members_device and the unpack of its frame, members of 64 KiB at width 1, beside bwts_pack_device_v(version 2,
      B = 64 KiB) and its unpack: the same stages;
  (c) --members members of mixed lengths (4 KiB to 4 MiB, log-uniform) and widths cycling 1, 2, 4, 8 in one call, beside one
      bwts_pack_planes_device / bwts_pack_device_v(version 2) call per member on the same context: the sum of the calls' total_ms, the
      wall time of the loop, and the packed sizes (--reps-c rounds: a round of the loop is thousands of calls).
    python tools/time_members.py [--log2n 30] [--reps 6] [--members 4096] [--reps-c 6] > profiles/members_stage.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402

SEG = 64 << 10


def spread(v):
    return max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--reps-c", type=int, default=6)
    ap.add_argument("--parts", default="abc")
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 6)
    pkg = ge.load_package()
    count = max(n // SEG, 1)
    ls = [min(n, SEG)] * count
    with pkg.Context(0) as ctx:
        if "a" in args.parts:
            x, y, back = (ctx.alloc(n) for _ in range(3))
            ctx.generate("zipf", 1, n, x)
            all4, cyc = [4] * count, [(1, 2, 4, 8)[k % 4] for k in range(count)]
            q = max(count // 4, 1)
            calls = [("split_segments (uniform, 4)", lambda: ctx.planes_split_segments_device(x, ls, 4, y)),
                     ("split_segments_w (all 4)", lambda: ctx.planes_split_segments_w_device(x, ls, all4, y)),
                     ("join_segments (uniform, 4)", lambda: ctx.planes_join_segments_device(y, ls, 4, back)),
                     ("join_segments_w (all 4)", lambda: ctx.planes_join_segments_w_device(y, ls, all4, back))]
            rounds(ctx, calls, 1)
            assert ctx.device_equal(back, x, n), "join(split(x)) != x at width 4"
            print("(a) zipf 2^%d as %d segments of %d bytes: %d rounds, the calls alternated" % (args.log2n, count, ls[0], reps))
            ts = rounds(ctx, calls, reps)
            m = report(ts)
            for d in ("split", "join"):
                u, w = "%s_segments (uniform, 4)" % d, "%s_segments_w (all 4)" % d
                print("  %s: mixed kernel / uniform kernel at width 4 = %.4f (%.3f vs %.3f ms; spread between rounds %.3f and %.3f ms); %.0f GB/s"
                      % (d, m[w] / m[u], m[w], m[u], spread(ts[w]), spread(ts[u]), 2 * n / m[w] / 1e6), flush=True)
            calls = [("split_segments_w (1,2,4,8)", lambda: ctx.planes_split_segments_w_device(x, ls, cyc, y)),
                     ("join_segments_w (1,2,4,8)", lambda: ctx.planes_join_segments_w_device(y, ls, cyc, back)),
                     ("device copy (one piece)", lambda: ctx.debug_copy_pieces(x, n, [(0, 0, n)], y, n))]
            calls += [("split_segments (uniform, %d), n/4" % w, (lambda w: lambda: ctx.planes_split_segments_device(x, ls[:q], w, y))(w)) for w in (2, 4, 8)]
            calls += [("device copy, n/4", lambda: ctx.debug_copy_pieces(x, n // 4, [(0, 0, n // 4)], y, n // 4))]
            rounds(ctx, calls[:2], 1)
            assert ctx.device_equal(back, x, n), "join(split(x)) != x at mixed widths"
            rounds(ctx, calls[2:], 1)
            print("(a) the widths cycling 1, 2, 4, 8 over the same segments")
            ts = rounds(ctx, calls, reps)
            m = report(ts)
            per_class = sum(m["split_segments (uniform, %d), n/4" % w] for w in (2, 4, 8)) + m["device copy, n/4"]
            print("  split at mixed widths / device copy = %.4f (%.3f vs %.3f ms); join / device copy = %.4f; one launch per width class: %.3f ms "
                  "in four calls (their total_ms added)" % (m["split_segments_w (1,2,4,8)"] / m["device copy (one piece)"], m["split_segments_w (1,2,4,8)"],
                                                             m["device copy (one piece)"], m["join_segments_w (1,2,4,8)"] / m["device copy (one piece)"], per_class), flush=True)
            for d in (x, y, back):
                d.free()

        if "b" in args.parts:
            cap = pkg.pack_members_bound(ls)
            x, back, f, g = ctx.alloc(n), ctx.alloc(n), ctx.alloc(cap), ctx.alloc(cap)
            ctx.generate("zipf", 1, n, x)
            size = {}
            calls = [("pack_device_v (2, 64 KiB)", lambda: size.update(v2=ctx.pack_device(x, n, SEG, g, cap, version=2))),
                     ("pack_members_device", lambda: size.update(m=ctx.pack_members_device(x, ls, None, f, cap))),
                     ("unpack_device (version 2)", lambda: ctx.unpack_device(g, size["v2"], back, n)),
                     ("unpack_device (members)", lambda: ctx.unpack_device(f, size["m"], back, n))]
            rounds(ctx, calls, 1)
            assert ctx.device_equal(back, x, n), "unpack(pack_members(x)) != x"
            assert size["m"] == size["v2"], size
            print("(b) zipf 2^%d as %d members of %d bytes at width 1, beside the version-2 frame at B = %d: %d rounds, the calls alternated; "
                  "both frames %d bytes, packed / n = %.4f" % (args.log2n, count, ls[0], ls[0], reps, size["m"], size["m"] / n))
            ts = rounds(ctx, calls, reps)
            m = report(ts)
            print("  pack: members / version 2 = %.4f (spread between rounds %.3f and %.3f ms); unpack: %.4f (spread %.3f and %.3f ms)"
                  % (m["pack_members_device"] / m["pack_device_v (2, 64 KiB)"], spread(ts["pack_members_device"]), spread(ts["pack_device_v (2, 64 KiB)"]),
                     m["unpack_device (members)"] / m["unpack_device (version 2)"], spread(ts["unpack_device (members)"]), spread(ts["unpack_device (version 2)"])), flush=True)
            for d in (x, back, f, g):
                d.free()

        if "c" in args.parts:
            rng = np.random.default_rng(1)
            mls = [int(v) for v in np.exp(rng.uniform(np.log(4 << 10), np.log(4 << 20), args.members))]
            mws = [(1, 2, 4, 8)[k % 4] for k in range(len(mls))]
            total = sum(mls)
            assert total <= 1 << 32
            cap = pkg.pack_members_bound(mls)
            x, back, f, g = ctx.alloc(total), ctx.alloc(total), ctx.alloc(cap), ctx.alloc(pkg.pack_bound(max(mls), 0, version=2) + 64)
            ctx.generate("zipf", 1, total, x)
            offs = np.concatenate(([0], np.cumsum(mls)[:-1])).tolist()
            res = {}

            def one_call():
                t0 = time.perf_counter()
                res["size"] = ctx.pack_members_device(x, mls, mws, f, cap)
                res["wall"] = (time.perf_counter() - t0) * 1e3
                res["ms"] = ctx.timings().total_ms

            def per_member():
                t0 = time.perf_counter()
                ms = size = 0
                for at, ln, w in zip(offs, mls, mws):
                    if w == 1:
                        size += ctx.pack_device(x.ptr + at, ln, 0, g, g.nbytes, version=2)
                    else:
                        size += ctx.pack_device(x.ptr + at, ln, 0, g, g.nbytes, planes=w)
                    ms += ctx.timings().total_ms
                res["loop_wall"] = (time.perf_counter() - t0) * 1e3
                res["loop_ms"], res["loop_size"] = ms, size

            one_call()
            assert ctx.unpack_device(f, res["size"], back, total) == total and ctx.device_equal(back, x, total), "unpack(pack_members(x)) != x"
            print("(c) %d members of %d bytes in all (4 KiB to 4 MiB, log-uniform, zipf), the widths cycling 1, 2, 4, 8: %d rounds, the two sides alternated"
                  % (len(mls), total, args.reps_c), flush=True)
            rows = []
            for _ in range(max(args.reps_c, 1)):
                one_call()
                per_member()
                rows.append(dict(res))
                print("  one call %.3f ms (wall %.3f); one call per member: total_ms added %.3f, wall %.3f" % (res["ms"], res["wall"], res["loop_ms"], res["loop_wall"]), flush=True)
            a, b = min(r["ms"] for r in rows), min(r["loop_ms"] for r in rows)
            print("  min: one call %.3f ms, one call per member %.3f ms (wall %.3f): %.1f times; packed %d bytes in one frame (%.4f of the input), "
                  "%d bytes in %d frames (%.4f)" % (a, b, min(r["loop_wall"] for r in rows), b / a, res["size"], res["size"] / total, res["loop_size"], len(mls),
                                                   res["loop_size"] / total), flush=True)
            one_call()
            calls = [("unpack_device (members)", lambda: ctx.unpack_device(f, res["size"], back, total)),
                     ("unpack_members_device (64 of them)", lambda: ctx.unpack_members_device(f, res["size"], list(range(0, len(mls), max(len(mls) // 64, 1)))[:64], back, total))]
            rounds(ctx, calls, 1)
            report(rounds(ctx, calls, max(args.reps_c, 1)))
            for d in (x, back, f, g):
                d.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
