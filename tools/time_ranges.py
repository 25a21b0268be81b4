"""Manual timing (GPU box) of copy_pieces_kernel and of range reads of a packed frame (include/bwts_pack.h, "Ranges"), in one process,
all times total_ms of the call, every call warmed up, then the calls alternated and the minimum of --reps rounds each.  Two bars, both
sides from this run; exit code 1 when one is missed:
  pieces  one piece of 2^30 - 16 bytes through bwts_debug_copy_pieces costs no more than bwts_planes_split_device at width 4 of the
          same bytes: both sides on 16-byte boundaries, the source one byte off, the destination one byte off, each against the
          split with the same side off.  (The split does strictly more per byte: byte permutes and a trip through the LDS.)
  whole   on the bench default zipf(2^30, seed 1) packed as version 2 in blocks of 64 KiB, reading the whole input as one range costs
          no more than (bwts_unpack_device of the same frame + the aligned copy_pieces above) x 1.05: the stages are the same, the
          cut-out is the one pass more, and the 5 % are for the table traffic.
For the record, with no bar: a plain device-to-device copy of the same bytes; one call with 1, 16, 256 and 4096 seeded random ranges
of 4 KiB, and the same ranges as one call each (the sum of the calls' total_ms, and the wall time around them).
    python tools/time_ranges.py [--log2n 30] [--reps 6] [--pieces-only] > profiles/ranges_stage.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch        # before the engine's library, as in bench.py: the HIP runtime that torch loads is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import pack_range_model as R  # noqa: E402
from time_ec import report, rounds  # noqa: E402
from time_planes import bar, device_copy_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--pieces-only", action="store_true", help="the kernel's table alone")
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 6)
    pkg = ge.load_package()
    ok = True
    with pkg.Context(0) as ctx:
        blk = min(n, 64 << 10)
        cap = pkg.pack_bound(n, blk, version=2)
        x, back, f = ctx.alloc(n), ctx.alloc(n), ctx.alloc(cap)
        ctx.generate("zipf", 1, n, x)
        m = n - 16

        # -- the kernel alone: one piece, beside the split at width 4 with the same side off a boundary -----------------------
        def pieces(s, d):
            return lambda: ctx.debug_copy_pieces(x, n, [(s, d, m)], back, n)

        calls = [("copy_pieces", pieces(0, 0)), ("planes_split_device w=4", lambda: ctx.planes_split_device(x, m, 4, back)),
                 ("copy_pieces, in + 1", pieces(1, 0)), ("planes_split_device w=4, in + 1", lambda: ctx.planes_split_device(x.ptr + 1, m, 4, back)),
                 ("copy_pieces, out + 1", pieces(0, 1)), ("planes_split_device w=4, out + 1", lambda: ctx.planes_split_device(x, m, 4, back.ptr + 1))]
        rounds(ctx, calls, 1)
        print("one piece of 2^%d - 16 bytes, T = %d: %d rounds, the six calls alternated" % (args.log2n, R.T, reps))
        t = report(rounds(ctx, calls, reps))
        for side in ("", ", in + 1", ", out + 1"):
            a, b = t["copy_pieces" + side], t["planes_split_device w=4" + side]
            ok &= bar("copy_pieces%s <= planes_split_device w=4%s" % (side, side), a <= b, a, b)
            print("    %.0f GB/s read + written" % (2 * m / a / 1e6))
        ctx.set_timing(2)
        for side, (sa, da) in (("", (0, 0)), (", in + 1", (1, 0)), (", out + 1", (0, 1))):
            pieces(sa, da)()
            print("  copy_pieces%s with per-kernel events: total %.3f ms, the kernel %s" % (side, ctx.timings().total_ms, " ".join("%.3f" % v for v in ctx.debug_last_spans())))
        ctx.set_timing(0)
        copy = device_copy_ms(n, reps)
        print("  plain device-to-device copy of 2^%d bytes (no bar): min %.3f ms (%s)" % (args.log2n, min(copy), " ".join("%.3f" % v for v in copy)), flush=True)
        aligned = t["copy_pieces"]
        if args.pieces_only:
            return 0 if ok else 1

        # -- the whole input as one range, beside the full unpack -----------------------------------------------------------
        size = ctx.pack_device(x, n, blk, f, cap, version=2)
        calls = [("unpack_device", lambda: ctx.unpack_device(f, size, back, n)),
                 ("unpack_ranges_device, (0, n)", lambda: ctx.unpack_ranges_device(f, size, [(0, n)], back, n))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, x, n), "the whole input read as one range is not the input"
        rep = ctx.debug_unpack_ranges_report()
        print("zipf 2^%d, seed 1, version 2 in %d blocks of 64 KiB, %d bytes: %d rounds, the two calls alternated" % (args.log2n, n // blk, size, reps))
        t = report(rounds(ctx, calls, reps))
        limit = 1.05 * (t["unpack_device"] + aligned)
        ok &= bar("unpack_ranges_device (0, n) <= 1.05 (unpack_device + copy_pieces)", t["unpack_ranges_device, (0, n)"] <= limit, t["unpack_ranges_device, (0, n)"], limit)
        print("    stages %s, %d covered blocks in %d run, device_bytes %d" % (" ".join(rep["stages"]), rep["blocks"], rep["runs"], ctx.timings().device_bytes), flush=True)

        # -- random ranges of 4 KiB: one call, and one call each (no bar) ------------------------------------------------------
        rng = np.random.default_rng(1)
        print("seeded random ranges of 4096 bytes of the same frame (no bar): one call with all of them, and one call each")
        print("  %6s %10s %10s %12s %14s %16s %14s" % ("ranges", "blocks", "runs", "one call ms", "each: sum ms", "each: wall ms", "rounds (each)"))
        for k in (1, 16, 256, 4096):
            rs = [(int(o), 4096) for o in rng.integers(0, n - 4096, k)]
            one = []
            for _ in range(reps + 1):
                ctx.unpack_ranges_device(f, size, rs, back, 4096 * k)
                one.append(ctx.timings().total_ms)
            rep = ctx.debug_unpack_ranges_report()
            each_rounds = reps if k <= 256 else 2
            sums, walls = [], []
            for _ in range(each_rounds + 1):
                s, t0 = 0.0, time.perf_counter()
                for i, r in enumerate(rs):
                    ctx.unpack_ranges_device(f, size, [r], back.ptr + 4096 * i, 4096)
                    s += ctx.timings().total_ms
                walls.append(1e3 * (time.perf_counter() - t0))
                sums.append(s)
            print("  %6d %10d %10d %12.3f %14.3f %16.3f %14d" % (k, rep["blocks"], rep["runs"], min(one[1:]), min(sums[1:]), min(walls[1:]), each_rounds), flush=True)
        for d in (x, back, f):
            d.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
