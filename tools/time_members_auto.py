"""Manual timing (GPU box) of the estimate and of the pack that chooses (include/bwts_members.h, "The estimate", "AUTO"), in one process,
everything resident in HBM, all times total_ms of the call: every call warmed up, then the calls alternated and the minimum of --reps
rounds each.  No bars: the figures are for the record.
  (1) the set of tools/time_members_direct.py, part 1: --members bf16 gaussian members (4 KiB to 4 MiB, log-uniform, scaled to 2^log2n
      bytes in all) at width 2: bwts_members_estimate_device beside bwts_planes_split_segments_w_device (one read and one write of the
      same bytes), the explicit all-direct and all-chain packs, the pack with the filters open and every method direct (expected: the
      all-direct pack plus the estimate), and the pack with the methods open at filter 0 (expected: the two explicit packs together);
      what lies above an expectation by more than the rounds' spread is shown stage by stage (timing level 2);
  (2) the estimate of one member of 2^log2n bytes at width 4 that holds one value -- every thread's run ends once, the contended path
      of a plain histogram -- beside the same member of noise.
    python tools/time_members_auto.py [--log2n 30] [--reps 6] [--members 4096] > profiles/members_auto.txt"""
import argparse
import os
import sys

import numpy as np
import torch        # before the engine's library, as in bench.py: the HIP runtime that torch loads is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402
from time_members_direct import bf16_weights, mix, spread  # noqa: E402


def stages(ctx, name, fn):
    """one more call at timing level 2: the device time of every timed launch, in launch order"""
    ctx.set_timing(2)
    fn()
    spans = ctx.debug_last_spans()
    ctx.set_timing(0)
    print("  %s, launch by launch (ms): %s; their sum %.3f of %.3f" % (name, " ".join("%.3f" % s for s in spans), sum(spans), ctx.timings().total_ms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--parts", default="12")
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 3)
    torch.cuda.init()
    pkg = ge.load_package()
    AUTO = pkg.METHOD_AUTO
    with pkg.Context(0) as ctx:
        if "1" in args.parts:
            ls = mix(args.members, n)
            ws = [2] * len(ls)
            direct, chain, open_ = [1] * len(ls), [0] * len(ls), [AUTO] * len(ls)
            cap = pkg.pack_members_bound_auto(ls, ws, open_)
            x, y, f = ctx.alloc(n), ctx.alloc(n), ctx.alloc(cap)
            bf16_weights(ctx, x, n)
            size, chose = {}, {}

            def auto(key, filters, methods):
                size[key], chose[key + " filters"], chose[key + " methods"] = ctx.pack_members_auto_device(x, ls, ws, f, cap, filters, methods)

            calls = [("members_estimate", lambda: ctx.members_estimate_device(x, ls, ws)),
                     ("planes_split_segments_w", lambda: ctx.planes_split_segments_w_device(x, ls, ws, y)),
                     ("pack, all direct", lambda: size.update(d=ctx.pack_members_device(x, ls, ws, f, cap, methods=direct))),
                     ("pack, all chain", lambda: size.update(c=ctx.pack_members_device(x, ls, ws, f, cap, methods=chain))),
                     ("pack, filters open, direct", lambda: auto("fo", open_, direct)),
                     ("pack, methods open", lambda: auto("mo", chain, open_))]
            rounds(ctx, calls, 1)
            e0, e1 = ctx.members_estimate_device(x, ls, ws)
            print("(1) %d bf16 gaussian members of %d bytes in all (4 KiB to 4 MiB), width 2: %d rounds, the calls alternated" % (len(ls), n, reps))
            print("  estimates: %d bytes without a filter, %d with delta; the all-direct frame %d, the all-chain frame %d" % (sum(e0), sum(e1), size["d"], size["c"]))
            print("  filters open: %d of %d members get delta, frame %d; methods open: %d of %d members direct, frame %d" %
                  (sum(chose["fo filters"]), len(ls), size["fo"], sum(chose["mo methods"]), len(ls), size["mo"]), flush=True)
            ts = rounds(ctx, calls, reps)
            m = report(ts)
            print("  the estimate: %.3f ms, %.1f GB/s; %.3f of the split, %.3f of the all-direct pack it advises" %
                  (m["members_estimate"], n / m["members_estimate"] / 1e6, m["members_estimate"] / m["planes_split_segments_w"], m["members_estimate"] / m["pack, all direct"]))
            want = m["pack, all direct"] + m["members_estimate"]
            over = m["pack, filters open, direct"] - want
            noise = max(spread(ts["pack, filters open, direct"]), spread(ts["pack, all direct"]), spread(ts["members_estimate"]))
            print("  filters open: %.3f ms; the all-direct pack and the estimate together %.3f ms: %+.3f ms (%.3f), the rounds' spread %.3f ms" %
                  (m["pack, filters open, direct"], want, over, m["pack, filters open, direct"] / want, noise), flush=True)
            if over > noise:
                stages(ctx, "filters open", calls[4][1])
                stages(ctx, "all direct", calls[2][1])
            want = m["pack, all direct"] + m["pack, all chain"]
            over = m["pack, methods open"] - want
            print("  methods open: %.3f ms; the all-chain and the all-direct pack together %.3f ms: %+.3f ms (%.3f)" %
                  (m["pack, methods open"], want, over, m["pack, methods open"] / want), flush=True)
            if over > 0.14 * want:
                stages(ctx, "methods open", calls[5][1])
                stages(ctx, "all chain", calls[3][1])
            for d in (x, y, f):
                d.free()
        if "2" in args.parts:
            x = ctx.alloc(n)
            out = {}
            for name, fill in (("one value", lambda: torch.full((n // 4,), 0x3F800000, dtype=torch.int32, device="cuda")),
                               ("noise", lambda: torch.randint(-(1 << 31), (1 << 31) - 1, (n // 4,), dtype=torch.int32, device="cuda"))):
                t = fill()
                torch.cuda.synchronize()
                ctx.debug_copy_pieces(t.data_ptr(), n, [(0, 0, n)], x.ptr, n)
                del t
                calls = [("members_estimate, " + name, lambda: out.update({name: ctx.members_estimate_device(x, [n], [4])}))]
                rounds(ctx, calls, 1)
                out[name + " ms"] = report(rounds(ctx, calls, reps))["members_estimate, " + name]
            print("(2) one member of %d bytes at width 4: one value %.3f ms (estimates %d and %d), noise %.3f ms (estimates %d and %d): %.3f" %
                  (n, out["one value ms"], out["one value"][0][0], out["one value"][1][0], out["noise ms"], out["noise"][0][0], out["noise"][1][0],
                   out["one value ms"] / out["noise ms"]), flush=True)
            x.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
