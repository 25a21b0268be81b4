"""Manual timing (GPU box) of the direct method of the member frame (include/bwts_members.h, version 3), in one process, everything
resident in HBM, all times total_ms of the call: every call warmed up, then the calls alternated and the minimum of --reps rounds
each.  No bars: the figures are for the record.
  (1) --members bf16 gaussian members (4 KiB to 4 MiB, log-uniform, scaled to 2^log2n bytes in all) at width 2, every member direct:
      bwts_pack_members_m_device and bwts_unpack_device, beside the same stages issued one after another -- bwts_crc32_segments_device,
      bwts_planes_split_segments_w_device, bwts_ec_encode_segments_device over the coder segments of the cut rule, and
      bwts_ec_decode_segments_device, bwts_planes_join_segments_w_device, bwts_crc32_segments_device back;
  (2) the same members, every second one direct (half the bytes within a few percent), beside the method-0 frame of the same members:
      times and sizes;
  (3) the method-0 member frame of --members zipf members with the widths cycling 1, 2, 4, 8 (tools/time_members.py, part c), this
      build beside the build of --parent (the directory of a bijective-bwt_amd package of the parent commit, built), alternated.
  The sizes of the two rows that the model pins (256 KiB of bf16 gaussian weights, and of the int32 walk), from the device's frames.
    python tools/time_members_direct.py [--log2n 30] [--reps 6] [--members 4096] [--parent DIR] > profiles/members_direct.txt"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch        # before the engine's library, as in bench.py: the HIP runtime that torch loads is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402

PLANE_MIN = 8192


def spread(v):
    return max(v) - min(v)


def cut(ln, w):
    """the coder segments of a direct member (members_plan.h: members_direct_segment_bytes)"""
    q = ln // w
    return [q] * (w - 1) + [q + ln - q * w] if w > 1 and q >= PLANE_MIN else [ln]


def mix(members, total):
    """--members even lengths, 4 KiB to 4 MiB log-uniform, scaled so that they add up to `total` bytes"""
    rng = np.random.default_rng(1)
    ls = np.exp(rng.uniform(np.log(4 << 10), np.log(4 << 20), members))
    ls = np.maximum((ls * (total / ls.sum())).astype(np.int64) & ~1, 4096)
    ls[int(ls.argmax())] += total - int(ls.sum())       # (the rounding's rest goes to the longest member)
    assert int(ls.min()) >= 4096 and int(ls.sum()) == total
    return [int(v) for v in ls]


def bf16_weights(ctx, x, n):
    """n bytes of bfloat16 gaussian weights (sigma 0.02) made on the device, into x"""
    piece = 1 << 27
    for at in range(0, n, piece):
        m = min(piece, n - at)
        t = ((torch.randn(m // 2, device="cuda") * 0.02).view(torch.int32) >> 16).to(torch.int16)
        torch.cuda.synchronize()
        ctx.debug_copy_pieces(t.data_ptr(), m, [(0, 0, m)], x.ptr + at, m)
        del t


def pinned_rows(ctx, pkg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pack_members_v2_model as M2
    print("the rows the model pins, 256 KiB each, member frames of one member from the device (stream bytes: the frame less header, entry and table)")
    for name, data, w in (("bf16 gaussian weights", M2.bf16_gaussian(), 2), ("i32 random walk", M2.walk_i32(), 4)):
        n = len(data)
        x, f = ctx.alloc(n), ctx.alloc(pkg.pack_members_bound([n], [w], [1]))
        x.upload(np.frombuffer(data, dtype=np.uint8))
        chain = ctx.pack_members_device(x, [n], [w], f, f.nbytes, methods=[0])
        direct = ctx.pack_members_device(x, [n], [w], f, f.nbytes, methods=[1])
        print("  %-24s width %d: chain %d (streams %d), direct %d (streams %d): %.4f" % (name, w, chain, chain - 64, direct, direct - 64 - 8 * w, direct / chain), flush=True)
        x.free()
        f.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parts", default="0123")
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 3)
    torch.cuda.init()
    pkg = ge.load_package()
    with pkg.Context(0) as ctx:
        if "0" in args.parts:
            pinned_rows(ctx, pkg)
        if "1" in args.parts or "2" in args.parts:
            ls = mix(args.members, n)
            ws = [2] * len(ls)
            segs = [s for ln in ls for s in cut(ln, 2)]
            direct, half, none = [1] * len(ls), [k & 1 for k in range(len(ls))], [0] * len(ls)
            cap = max(pkg.pack_members_bound(ls, ws, direct), pkg.pack_members_bound(ls))
            x, y, back, f, g = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(cap), ctx.alloc(cap)
            bf16_weights(ctx, x, n)
            size = {}
        if "1" in args.parts:
            calls = [("pack_members_m_device", lambda: size.update(d=ctx.pack_members_device(x, ls, ws, f, cap, methods=direct))),
                     ("unpack_device", lambda: ctx.unpack_device(f, size["d"], back, n)),
                     ("crc32_segments", lambda: ctx.crc32_segments_device(x, ls)),
                     ("planes_split_segments_w", lambda: ctx.planes_split_segments_w_device(x, ls, ws, y)),
                     ("ec_encode_segments", lambda: size.update(s=ctx.ec_encode_segments_device(y, segs, g, cap))),
                     ("ec_decode_segments", lambda: ctx.ec_decode_segments_device(g, size["s"], segs, y)),
                     ("planes_join_segments_w", lambda: ctx.planes_join_segments_w_device(y, ls, ws, back)),
                     ("crc32_segments (back)", lambda: ctx.crc32_segments_device(back, ls))]
            rounds(ctx, calls, 1)
            assert ctx.device_equal(back, x, n), "the stages one after another do not give the input back"
            ctx.unpack_device(f, size["d"], back, n)
            assert ctx.device_equal(back, x, n), "unpack(pack_members_m(x)) != x"
            assert int(size["s"].sum()) == size["d"] - 32 - 32 * len(ls) - 8 * sum(2 for ln in ls if len(cut(ln, 2)) > 1)
            print("(1) %d bf16 gaussian members of %d bytes in all (4 KiB to 4 MiB), width 2, all direct, %d coder segments: %d rounds, the calls "
                  "alternated; frame %d bytes, %.4f of the input" % (len(ls), n, len(segs), reps, size["d"], size["d"] / n), flush=True)
            m = report(rounds(ctx, calls, reps))
            enc = m["crc32_segments"] + m["planes_split_segments_w"] + m["ec_encode_segments"]
            dec = m["ec_decode_segments"] + m["planes_join_segments_w"] + m["crc32_segments (back)"]
            print("  pack: one call %.3f ms, the three stages %.3f ms: %.3f; unpack: one call %.3f ms, the three stages %.3f ms: %.3f; %.1f and %.1f GB/s"
                  % (m["pack_members_m_device"], enc, m["pack_members_m_device"] / enc, m["unpack_device"], dec, m["unpack_device"] / dec,
                     n / m["pack_members_m_device"] / 1e6, n / m["unpack_device"] / 1e6), flush=True)
        if "2" in args.parts:
            calls = [("pack, every second direct", lambda: size.update(h=ctx.pack_members_device(x, ls, ws, f, cap, methods=half))),
                     ("unpack, every second direct", lambda: ctx.unpack_device(f, size["h"], back, n)),
                     ("pack, method 0", lambda: size.update(c=ctx.pack_members_device(x, ls, ws, g, cap, methods=none))),
                     ("unpack, method 0", lambda: ctx.unpack_device(g, size["c"], back, n))]
            rounds(ctx, calls[:2], 1)
            assert ctx.device_equal(back, x, n), "unpack(pack(x)) != x, mixed frame"
            rounds(ctx, calls[2:], 1)
            assert ctx.device_equal(back, x, n), "unpack(pack(x)) != x, method-0 frame"
            db = sum(ln for ln, h in zip(ls, half) if h)
            print("(2) the same members, every second one direct (%d of %d bytes), beside the method-0 frame: %d rounds; frames %d and %d bytes, "
                  "%.4f and %.4f of the input" % (db, n, reps, size["h"], size["c"], size["h"] / n, size["c"] / n), flush=True)
            report(rounds(ctx, calls, reps))
        if "1" in args.parts or "2" in args.parts:
            for d in (x, y, back, f, g):
                d.free()

        if "3" in args.parts:
            rng = np.random.default_rng(1)
            mls = [int(v) for v in np.exp(rng.uniform(np.log(4 << 10), np.log(4 << 20), args.members))]
            mws = [(1, 2, 4, 8)[k % 4] for k in range(len(mls))]
            total = sum(mls)
            cap = pkg.pack_members_bound(mls)
            x, back, f = ctx.alloc(total), ctx.alloc(total), ctx.alloc(cap)
            ctx.generate("zipf", 1, total, x)
            size = {}
            calls = [("this build: pack", lambda: size.update(a=ctx.pack_members_device(x, mls, mws, f, cap))),
                     ("this build: unpack", lambda: ctx.unpack_device(f, size["a"], back, total))]
            print("(3) the method-0 frame of %d zipf members, %d bytes in all, widths cycling 1, 2, 4, 8" % (len(mls), total), flush=True)
            if args.parent:
                spec = importlib.util.spec_from_file_location("bwts_parent", os.path.join(args.parent, "__init__.py"), submodule_search_locations=[args.parent])
                parent = importlib.util.module_from_spec(spec)
                sys.modules["bwts_parent"] = parent
                spec.loader.exec_module(parent)
                with parent.Context(0) as pctx:
                    pcalls = [("parent: pack", lambda: size.update(b=pctx.pack_members_device(x.ptr, mls, mws, f.ptr, cap))),
                              ("parent: unpack", lambda: pctx.unpack_device(f.ptr, size["b"], back.ptr, total))]
                    for _ in range(2):
                        for (_, fn), (_, pfn) in zip(calls, pcalls):
                            fn()
                            pfn()
                    assert size["a"] == size["b"] and ctx.device_equal(back, x, total)
                    ts = {name: [] for name, _ in calls + pcalls}
                    for _ in range(reps):
                        for (name, fn), (pname, pfn) in zip(calls, pcalls):
                            fn()
                            ts[name].append(ctx.timings().total_ms)
                            pfn()
                            ts[pname].append(pctx.timings().total_ms)
                    m = report(ts)
                    for d in ("pack", "unpack"):
                        a, b = "this build: %s" % d, "parent: %s" % d
                        print("  %s: this build / parent = %.4f (spread between rounds %.3f and %.3f ms); frame %d bytes both" %
                              (d, m[a] / m[b], spread(ts[a]), spread(ts[b]), size["a"]), flush=True)
            else:
                rounds(ctx, calls, 1)
                report(rounds(ctx, calls, reps))
            for d in (x, back, f):
                d.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
