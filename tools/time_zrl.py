"""Manual timing (GPU box) of the zero-run stage beside the move-to-front stage and the coder, and of pack / unpack with frames of
version 2 beside the single calls they chain, in one process, all times total_ms of the call: every call warmed up, then the calls
alternated and the minimum of --reps rounds each.  The bars, both sides from this run, no further margin; exit code 1 when one is
missed:
  stage   on the move-to-front ranks of the bench default zipf(2^30, seed 1) and of realtext.corpus(2^26): zrl_encode_device costs no
          more than mtf_forward_device, zrl_decode_device no more than mtf_inverse_device;
  pack    pack_device version 2 (one block) costs no more than forward_device + mtf_forward_device + zrl_encode_device +
          ec_encode_device over the run-coded bytes + one ec_encode_device over the ranks (the allowance version 1 has in
          tools/time_pack.py), and unpack_device no more than the mirror image;
  run     one rank and 2^30 - 1 zeros: encode and decode each cost no more than on the zipf ranks of the same length.
For the record, with no bar: the ratios to the coder's calls over the same ranks, the coder's time over the run-coded bytes, packed
size / n for zipf and the real-text corpus in one block and in 1 MiB blocks for both versions, and what the coder pays for byte-side
segments that start off 16 bytes (the concatenated zero-run outputs).
    python tools/time_zrl.py [--log2n 30] [--reps 6] > profiles/zrl_stage.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402


def bar(name, ok, a, b):
    print("  bar: %s: %s (%.3f vs %.3f)" % (name, "holds" if ok else "MISSED", a, b), flush=True)
    return ok


def stage(ctx, pkg, what, y, r, z, s, back, n, cap, reps, size):
    """the six stage calls over the ranks of the BWTS in y, alternated; -> the minima, the stage's two bars"""
    calls = [("mtf_forward_device", lambda: ctx.mtf_forward_device(y, n, r)),
             ("zrl_encode_device", lambda: size.update(m=ctx.zrl_encode_device(r, n, z, n))),
             ("ec_encode_device (ranks)", lambda: size.update(ranks=ctx.ec_encode_device(r, n, s, cap))),
             ("ec_decode_device (ranks)", lambda: ctx.ec_decode_device(s, size["ranks"], back, n)),
             ("ec_encode_device (coded)", lambda: size.update(coded=ctx.ec_encode_device(z, size["m"], s, cap))),
             ("ec_decode_device (coded)", lambda: ctx.ec_decode_device(s, size["coded"], back, size["m"])),
             ("zrl_decode_device", lambda: ctx.zrl_decode_device(z, size["m"], back, n)),
             ("mtf_inverse_device", lambda: ctx.mtf_inverse_device(r, n, back))]
    rounds(ctx, calls, 1)
    ctx.zrl_decode_device(z, size["m"], back, n)
    assert ctx.device_equal(back, r, n), "zrl_decode(zrl_encode(ranks)) != ranks"
    print("%s: %d rounds, the eight calls alternated" % (what, reps))
    m = report(rounds(ctx, calls, reps))
    ok = bar("zrl_encode_ms <= mtf_forward_ms", m["zrl_encode_device"] <= m["mtf_forward_device"], m["zrl_encode_device"], m["mtf_forward_device"])
    ok &= bar("zrl_decode_ms <= mtf_inverse_ms", m["zrl_decode_device"] <= m["mtf_inverse_device"], m["zrl_decode_device"], m["mtf_inverse_device"])
    print("  run-coded bytes m / n = %.4f; coder stream over the ranks %.4f n, over the run-coded bytes %.4f n" % (
        size["m"] / n, size["ranks"] / n, size["coded"] / n))
    print("  zrl_encode / ec_encode (ranks) = %.2f; zrl_decode / ec_decode (ranks) = %.2f; the coder over m bytes: %.3f / %.3f ms" % (
        m["zrl_encode_device"] / m["ec_encode_device (ranks)"], m["zrl_decode_device"] / m["ec_decode_device (ranks)"],
        m["ec_encode_device (coded)"], m["ec_decode_device (coded)"]), flush=True)
    ctx.set_timing(2)
    for name, fn, names in (("zrl_encode_device", lambda: ctx.zrl_encode_device(r, n, z, n), ["summaries", "max-scan", "sum-scan", "store"]),
                            ("zrl_decode_device", lambda: ctx.zrl_decode_device(z, size["m"], back, n), ["weights", "scan", "clear", "write"])):
        fn()
        print("  %s with per-kernel events: total %.3f ms: %s" % (name, ctx.timings().total_ms, ", ".join(
            "%s %.3f" % (k, ms) for k, ms in zip(names, ctx.debug_last_spans()))), flush=True)
    ctx.set_timing(0)
    return m, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--log2text", type=int, default=26)
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 6)
    pkg = ge.load_package()
    ok = True
    with pkg.Context(0) as ctx:
        mib = min(n, 1 << 20)
        cap = max(pkg.pack_bound(n, mib, version=2), pkg.pack_bound(n, 0, version=2))
        x, y, r, z, back = (ctx.alloc(n) for _ in range(5))
        s, f = ctx.alloc(cap), ctx.alloc(cap)
        size = {}

        # -- the stage beside move-to-front and the coder ---------------------------------------------------------
        ctx.generate("zipf", 1, n, x)
        ctx.forward_device(x, n, y)
        zipf, good = stage(ctx, pkg, "zipf 2^%d, seed 1 (the bench default), the move-to-front ranks" % args.log2n, y, r, z, s, back, n, cap, reps, size)
        ok &= good

        # -- pack and unpack, version 2, beside the calls they chain: one block ---------------------------------------
        calls = [("forward_device", lambda: ctx.forward_device(x, n, y)),
                 ("pack_device v2", lambda: size.update(frame=ctx.pack_device(x, n, 0, f, cap, version=2))),
                 ("inverse_device", lambda: ctx.inverse_device(y, n, back)),
                 ("unpack_device v2", lambda: ctx.unpack_device(f, size["frame"], back, n)),
                 ("pack_device v1", lambda: size.update(frame1=ctx.pack_device(x, n, 0, s, cap))),
                 ("unpack_device v1", lambda: ctx.unpack_device(s, size["frame1"], back, n))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, x, n), "unpack(pack(x)) != x"
        print("zipf 2^%d, one block: %d rounds, the six calls alternated" % (args.log2n, reps))
        m = report(rounds(ctx, calls, reps))
        chain_p = m["forward_device"] + zipf["mtf_forward_device"] + zipf["zrl_encode_device"] + zipf["ec_encode_device (coded)"] + zipf["ec_encode_device (ranks)"]
        chain_u = zipf["ec_decode_device (coded)"] + zipf["zrl_decode_device"] + zipf["mtf_inverse_device"] + m["inverse_device"] + zipf["ec_encode_device (ranks)"]
        ok &= bar("pack_v2_ms <= forward + mtf_forward + zrl_encode + ec_encode (coded) + ec_encode (ranks)", m["pack_device v2"] <= chain_p, m["pack_device v2"], chain_p)
        ok &= bar("unpack_v2_ms <= ec_decode (coded) + zrl_decode + mtf_inverse + inverse + ec_encode (ranks)", m["unpack_device v2"] <= chain_u, m["unpack_device v2"], chain_u)
        print("  packed / n: version 1 %.4f, version 2 %.4f" % (size["frame1"] / n, size["frame"] / n), flush=True)
        for v in (1, 2):
            got = ctx.pack_device(x, n, mib, f, cap, version=v)
            assert ctx.unpack_device(f, got, back, n) == n and ctx.device_equal(back, x, n)
            print("  in blocks of 1 MiB, version %d (no bar): packed / n = %.4f" % (v, got / n), flush=True)

        # -- one run: a fill done by one wave would show here ---------------------------------------------------------
        one = np.zeros(n, dtype=np.uint8)
        one[0] = 113
        r.upload(one)
        del one
        calls = [("zrl_encode_device", lambda: size.update(run=ctx.zrl_encode_device(r, n, z, n))),
                 ("zrl_decode_device", lambda: ctx.zrl_decode_device(z, size["run"], back, n))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, r, n)
        print("one rank and 2^%d - 1 zeros (%d coded bytes): %d rounds" % (args.log2n, size["run"], reps))
        m = report(rounds(ctx, calls, reps))
        ok &= bar("encode of one run <= encode of the zipf ranks", m["zrl_encode_device"] <= zipf["zrl_encode_device"], m["zrl_encode_device"], zipf["zrl_encode_device"])
        ok &= bar("decode of one run <= decode of the zipf ranks", m["zrl_decode_device"] <= zipf["zrl_decode_device"], m["zrl_decode_device"], zipf["zrl_decode_device"])

        # -- real text, where zero runs matter --------------------------------------------------------------------------
        import realtext
        text = np.frombuffer(realtext.corpus(min(1 << args.log2text, n)), dtype=np.uint8)
        tn = text.size
        x.upload(text)
        ctx.forward_device(x, tn, y)
        _, good = stage(ctx, pkg, "realtext.corpus %d bytes, the move-to-front ranks" % tn, y, r, z, s, back, tn, cap, reps, size)
        ok &= good
        for name, b in (("one block", 0), ("blocks of 1 MiB", min(tn, 1 << 20))):
            for v in (1, 2):
                got = ctx.pack_device(x, tn, b, f, cap, version=v)
                assert ctx.unpack_device(f, got, back, tn) == tn and ctx.device_equal(back, x, tn)
                print("  %s, version %d (no bar): packed %d bytes / n = %.4f" % (name, v, got, got / tn), flush=True)
        # the coder behind the concatenated zero-run segments: byte-side segments that start anywhere, beside as many of the same
        # bytes that start on multiples of 16
        blk = min(tn, 1 << 20)
        ls = np.full(tn // blk, blk, dtype=np.uint64)
        ctx.mtf_forward_segments_device(y, ls, r) if ls.size > 1 else ctx.mtf_forward_device(y, tn, r)
        if ls.size > 1:
            coded = ctx.zrl_encode_segments_device(r, ls, z, tn)
            even = np.full(ls.size, (int(coded.sum()) // ls.size) & ~15, dtype=np.uint64)
            calls = [("ec_encode_segments_device, starts anywhere", lambda: ctx.ec_encode_segments_device(z, coded, s, cap)),
                     ("ec_encode_segments_device, starts on 16", lambda: ctx.ec_encode_segments_device(z, even, s, cap))]
            rounds(ctx, calls, 1)
            print("the coder over %d zero-run coded segments (%d bytes; %d of them start off 16 bytes), beside %d segments of %d bytes (no bar)" % (
                ls.size, int(coded.sum()), int(np.count_nonzero(np.cumsum(coded)[:-1] % 16)), ls.size, int(even[0])))
            report(rounds(ctx, calls, reps))
        for d in (x, y, r, z, back, s, f):
            d.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
