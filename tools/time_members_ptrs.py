"""Manual timing (GPU box) of the member calls over tables of device pointers (include/bwts_members.h, "Pointers"),
in one process, everything resident in HBM, all times total_ms of the call: every call warmed up, then the calls alternated and the
minimum of --reps rounds each.  The input is the README's --members bf16 gaussian arrays (4 KiB to 4 MiB, 2^log2n bytes in all), every
array in an allocation of its own, and the same bytes back to back in one buffer.
  (1) bwts_gather_device and bwts_scatter_device alone, beside copy_pieces_kernel over the same bytes as one piece
      (bwts_debug_copy_pieces).  Bar: each at most 1.25 x the one-piece copy.
  (2) bwts_pack_members_p_device over the scattered arrays beside bwts_pack_members_a_device over the buffer, every member direct, and
      bwts_unpack_members_p_device into the scattered arrays beside bwts_unpack_members_device of every member into one buffer.
      Bar: a pointer call at most the contiguous call plus the measured gather (scatter), and 8 % of the sum for the spread between
      boxes.
The bars are printed as met or missed; they are not gates.
    python tools/time_members_ptrs.py [--log2n 30] [--reps 6] [--members 4096] > profiles/members_ptrs.txt"""
import argparse
import os
import sys

import torch        # before the engine's library, as in bench.py: the HIP runtime that torch loads is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402
from time_members_direct import bf16_weights, mix  # noqa: E402

SPREAD = 0.08


def bar(name, got, most):
    print("  %-44s %8.3f ms against %8.3f ms: %s (%.3f)" % (name, got, most, "met" if got <= most else "MISSED", got / most), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--members", type=int, default=4096)
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 3)
    torch.cuda.init()
    pkg = ge.load_package()
    with pkg.Context(0) as ctx:
        ls = mix(args.members, n)
        ws, direct, count = [2] * len(ls), [1] * len(ls), len(ls)
        cap = pkg.pack_members_bound(ls, ws, direct)
        x, back, f = ctx.alloc(n), ctx.alloc(n), ctx.alloc(cap)
        bf16_weights(ctx, x, n)
        own = [ctx.alloc(ln) for ln in ls]           # every array in an allocation of its own
        ctx.scatter_device(x, own, ls)
        ctx.gather_device(own, ls, back)
        assert ctx.device_equal(back, x, n), "gather(scatter(x)) != x"
        size = {}
        every = list(range(count))
        print("%d bf16 gaussian arrays of %d bytes in all (4 KiB to 4 MiB), each in an allocation of its own: %d rounds, the calls alternated"
              % (count, n, reps), flush=True)
        calls = [("gather_device", lambda: ctx.gather_device(own, ls, back)),
                 ("scatter_device", lambda: ctx.scatter_device(x, own, ls)),
                 ("copy_pieces, one piece", lambda: ctx.debug_copy_pieces(x, n, [(0, 0, n)], back, n))]
        rounds(ctx, calls, 1)
        print("(1) the copy between scattered buffers alone", flush=True)
        m = report(rounds(ctx, calls, reps))
        one = m["copy_pieces, one piece"]
        print("  %.1f, %.1f and %.1f GB/s of bytes copied" % tuple(n / m[k] / 1e6 for k in ("gather_device", "scatter_device", "copy_pieces, one piece")), flush=True)
        bar("gather <= 1.25 x the one-piece copy", m["gather_device"], 1.25 * one)
        bar("scatter <= 1.25 x the one-piece copy", m["scatter_device"], 1.25 * one)

        calls = [("pack_members_ptrs_device", lambda: size.update(p=ctx.pack_members_ptrs_device(own, ls, ws, f, cap, 0, direct)[0])),
                 ("pack_members_auto_device", lambda: size.update(a=ctx.pack_members_auto_device(x, ls, ws, f, cap, 0, direct)[0])),
                 ("unpack_members_ptrs_device", lambda: ctx.unpack_members_ptrs_device(f, size["a"], None, own, ls)),
                 ("unpack_members_device", lambda: ctx.unpack_members_device(f, size["a"], every, back, n))]
        rounds(ctx, calls, 1)
        assert size["p"] == size["a"] and ctx.device_equal(back, x, n)
        ctx.gather_device(own, ls, back)
        assert ctx.device_equal(back, x, n), "the arrays that unpack_members_ptrs_device wrote are not the input"
        print("(2) the member calls, every member direct at width 2; frame %d bytes, %.4f of the input; device_bytes %d" %
              (size["a"], size["a"] / n, ctx.timings().device_bytes), flush=True)
        p = report(rounds(ctx, calls, reps))
        print("  %.1f and %.1f GB/s through the pointer calls" % (n / p["pack_members_ptrs_device"] / 1e6, n / p["unpack_members_ptrs_device"] / 1e6), flush=True)
        bar("pack, pointers <= contiguous + gather + 8 %", p["pack_members_ptrs_device"], (1 + SPREAD) * (p["pack_members_auto_device"] + m["gather_device"]))
        bar("unpack, pointers <= contiguous + scatter + 8 %", p["unpack_members_ptrs_device"], (1 + SPREAD) * (p["unpack_members_device"] + m["scatter_device"]))
        for d in [x, back, f] + own:
            d.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
