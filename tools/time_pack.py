"""Manual timing (GPU box) of the checksum kernel and of pack / unpack beside the single calls they chain, in one process, all times
total_ms of the call: the bench default zipf(2^30, seed 1) generated on the device, every call warmed up, then the calls alternated and
the minimum of --reps rounds each.  Two bars, both sides from this run, no further margin; exit code 1 when one is missed:
  crc     bwts_crc32_device over the ranks costs no more than bwts_ec_encode_device of the same bytes;
  pack    bwts_pack_device (one block) costs no more than forward_device + mtf_forward_device + 2 x ec_encode_device issued one after
          another (the second encode is the allowance for the checksum pass), and bwts_unpack_device no more than ec_decode_device +
          mtf_inverse_device + inverse_device + one ec_encode_device.
Beside the times: the checksum's GB/s and per-launch spans, and without a bar the 64 KiB block form and packed size / n for zipf and
for the real-text corpus (tests/realtext.py).
    python tools/time_pack.py [--log2n 30] [--reps 6] > profiles/pack_stage.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402


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
        blk = min(n, 64 << 10)
        cap = max(pkg.pack_bound(n, blk), pkg.pack_bound(n))
        x, y, r, back = (ctx.alloc(n) for _ in range(4))
        s, f = ctx.alloc(cap), ctx.alloc(cap)
        size = {}
        ctx.generate("zipf", 1, n, x)
        ctx.forward_device(x, n, y)
        ctx.mtf_forward_device(y, n, r)

        # -- the checksum beside the coder, on the ranks --------------------------------------------------------
        calls = [("crc32_device", lambda: size.update(crc=ctx.crc32_device(r, n))),
                 ("ec_encode_device", lambda: size.update(one=ctx.ec_encode_device(r, n, s, cap)))]
        rounds(ctx, calls, 1)
        print("zipf 2^%d, seed 1 (the bench default), the move-to-front ranks: %d rounds, the two calls alternated" % (args.log2n, reps))
        m = report(rounds(ctx, calls, reps))
        good = m["crc32_device"] <= m["ec_encode_device"]
        ok &= good
        print("  bar: crc32_ms <= ec_encode_ms: %s (%.3f vs %.3f); the checksum reads %.0f GB/s (DESIGN section 4.1: a copy reaches about 6 TB/s "
              "counting both directions)" % ("holds" if good else "MISSED", m["crc32_device"], m["ec_encode_device"], n / m["crc32_device"] / 1e6), flush=True)
        ctx.set_timing(2)
        ctx.crc32_device(r, n)
        t = ctx.timings()
        names = ["tiles", "fold groups", "fold all"] if pkg.debug_crc_plan(n)["groups"] > 1 else ["tiles", "fold all"]
        print("  crc32_device with per-kernel events: total %.3f ms: %s" % (t.total_ms, ", ".join("%s %.3f" % (k, ms) for k, ms in zip(names, ctx.debug_last_spans()))))
        ctx.set_timing(0)

        # -- pack and unpack beside the calls they chain, one block ----------------------------------------------
        calls = [("forward_device", lambda: ctx.forward_device(x, n, y)),
                 ("mtf_forward_device", lambda: ctx.mtf_forward_device(y, n, r)),
                 ("ec_encode_device", lambda: size.update(one=ctx.ec_encode_device(r, n, s, cap))),
                 ("pack_device", lambda: size.update(frame=ctx.pack_device(x, n, 0, f, cap))),
                 ("ec_decode_device", lambda: ctx.ec_decode_device(s, size["one"], back, n)),
                 ("mtf_inverse_device", lambda: ctx.mtf_inverse_device(r, n, back)),
                 ("inverse_device", lambda: ctx.inverse_device(y, n, back)),
                 ("unpack_device", lambda: ctx.unpack_device(f, size["frame"], back, n))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, x, n), "unpack(pack(x)) != x"
        assert size["frame"] == 48 + size["one"]
        print("zipf 2^%d, one block: %d rounds, the eight calls alternated" % (args.log2n, reps))
        m = report(rounds(ctx, calls, reps))
        chain_p = m["forward_device"] + m["mtf_forward_device"] + 2 * m["ec_encode_device"]
        chain_u = m["ec_decode_device"] + m["mtf_inverse_device"] + m["inverse_device"] + m["ec_encode_device"]
        good_p, good_u = m["pack_device"] <= chain_p, m["unpack_device"] <= chain_u
        ok &= good_p and good_u
        print("  bar: pack_ms <= forward + mtf_forward + 2 ec_encode: %s (%.3f vs %.3f); unpack_ms <= ec_decode + mtf_inverse + inverse + ec_encode: "
              "%s (%.3f vs %.3f)" % ("holds" if good_p else "MISSED", m["pack_device"], chain_p, "holds" if good_u else "MISSED", m["unpack_device"], chain_u), flush=True)
        print("  packed %d bytes / n = %.4f" % (size["frame"], size["frame"] / n), flush=True)

        # -- for the record: blocks of 64 KiB ----------------------------------------------------------------------
        calls = [("pack_device", lambda: size.update(blocks=ctx.pack_device(x, n, blk, f, cap))),
                 ("unpack_device", lambda: ctx.unpack_device(f, size["blocks"], back, n))]
        rounds(ctx, calls, 1)
        assert ctx.device_equal(back, x, n)
        print("zipf 2^%d in %d blocks of 64 KiB (no bar): packed / n = %.4f" % (args.log2n, n // blk, size["blocks"] / n))
        report(rounds(ctx, calls, reps))

        # -- for the record: real text, where zero runs matter ------------------------------------------------------
        import realtext
        text = np.frombuffer(realtext.corpus(min(1 << args.log2text, n)), dtype=np.uint8)
        x.upload(text)
        for name, b in (("one block", 0), ("blocks of 1 MiB", 1 << 20)):
            got = ctx.pack_device(x, text.size, b, f, cap)
            assert ctx.unpack_device(f, got, back, text.size) == text.size and ctx.device_equal(back, x, text.size)
            print("realtext.corpus %d bytes, %s (no bar): packed %d bytes / n = %.4f" % (text.size, name, got, got / text.size), flush=True)
        for d in (x, y, r, back, s, f):
            d.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
