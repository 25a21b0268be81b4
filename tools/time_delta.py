"""Manual timing (GPU box) of the delta filter beside the zero-run stage and the byte-plane join, in one process, all times total_ms of
the call: every call warmed up, then the calls alternated and the minimum of --reps rounds each.  The bar, both sides from this run, no
further margin; exit code 1 when it is missed:
  stage   on 2^30 bytes resident in HBM, delta_encode_device and delta_decode_device at each width cost no more than
          zrl_encode_device on the move-to-front ranks of the bench default zipf(2^30, seed 1).
For the record, with no bar: planes_join_device at the same width beside each pair (width 1 has none); sides one byte off a 16-byte
boundary; the segment form on segments of 64 KiB with widths cycling 1, 2, 4, 8 and every third segment copied; packed size / n of the
device's member frames of one member with and without the filter for typed inputs of 256 KiB.
    python tools/time_delta.py [--log2n 30] [--reps 6] > profiles/delta_stage.txt"""
import argparse
import os
import sys

import numpy as np
import torch        # before the engine's library, as in bench.py: the HIP runtime that torch loads is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402
from time_planes import bar, field  # noqa: E402


def typed_inputs(nbytes):
    """(name, width, bytes): the rows of the size table, numpy default_rng(5)"""
    rng = np.random.default_rng(5)
    walk = np.cumsum(rng.integers(-50, 51, nbytes // 4)).astype("<i4").tobytes()
    rng = np.random.default_rng(5)
    g16 = (0.02 * rng.standard_normal(nbytes // 2)).astype("<f4")
    stamps = (1_700_000_000_000 + np.cumsum(rng.integers(900, 1101, nbytes // 8))).astype("<u8").tobytes()
    sensor = (2000 + 1500 * np.sin(np.arange(nbytes // 2) / 300.0) + rng.normal(0, 3, nbytes // 2)).astype("<u2").tobytes()
    ids = np.sort(rng.integers(0, 1 << 32, nbytes // 4, dtype=np.uint64)).astype("<u4").tobytes()
    return [("i32 random walk, steps +-50", 4, walk),
            ("i64 timestamps, steps 900..1100", 8, stamps),
            ("u16 smooth sensor + noise", 2, sensor),
            ("u32 sorted random ids", 4, ids),
            ("f32 smooth field (as integers)", 4, field(0, nbytes // 4, rng).tobytes()),
            ("bf16 gaussian weights", 2, (g16.view("<u4") >> 16).astype("<u2").tobytes())]


def size_table(ctx, pkg, x, f, back, nbytes):
    print("packed size / n, member frames of one member of %d bytes: planes at the width alone, and the delta filter in front of them" % nbytes)
    print("  %-34s %5s %11s %13s" % ("input (numpy, seeded)", "width", "planes only", "delta, planes"))
    for name, w, data in typed_inputs(nbytes):
        n = len(data)
        x.upload(np.frombuffer(data, dtype=np.uint8))
        sizes = []
        for flt in (0, 1):
            got = ctx.pack_members_device(x, [n], [w], f, pkg.pack_members_bound([n]), filters=[flt])
            assert ctx.unpack_device(f, got, back, n) == n and ctx.device_equal(back, x, n), (name, flt)
            sizes.append(got)
        print("  %-34s %5d %11.4f %13.4f   (%d -> %d bytes)" % (name, w, sizes[0] / n, sizes[1] / n, sizes[0], sizes[1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=6)
    args = ap.parse_args()
    n = 1 << args.log2n
    reps = max(args.reps, 6)
    torch.cuda.init()
    pkg = ge.load_package()
    ok = True
    with pkg.Context(0) as ctx:
        kib = min(n, 1 << 18)
        x, y, r, back = (ctx.alloc(n) for _ in range(4))
        f = ctx.alloc(pkg.pack_members_bound([kib]))

        size_table(ctx, pkg, x, f, back, kib)

        # -- the stage beside the zero-run stage: 2^30 bytes resident, the calls alternated -------------------------------------
        ctx.generate("zipf", 1, n, x)
        ctx.forward_device(x, n, y)
        ctx.mtf_forward_device(y, n, r)
        calls = [("zrl_encode_device (zipf ranks)", lambda: ctx.zrl_encode_device(r, n, y, n))]
        for w in (1, 2, 4, 8):
            calls.append(("delta_encode_device w=%d" % w, lambda w=w: ctx.delta_encode_device(x, n, w, back)))
            calls.append(("delta_decode_device w=%d" % w, lambda w=w: ctx.delta_decode_device(x, n, w, back)))
            if w > 1:
                calls.append(("planes_join_device w=%d" % w, lambda w=w: ctx.planes_join_device(x, n, w, back)))
        rounds(ctx, calls, 1)
        for w in (1, 2, 4, 8):
            ctx.delta_encode_device(x, n, w, back)
            ctx.delta_decode_device(back, n, w, y)
            assert ctx.device_equal(y, x, n), "decode(encode(x)) != x at width %d" % w
        print("zipf 2^%d, seed 1 (the bench default): %d rounds, the %d calls alternated" % (args.log2n, reps, len(calls)))
        m = report(rounds(ctx, calls, reps))
        zrl = m["zrl_encode_device (zipf ranks)"]
        for name, ms in m.items():
            if name.startswith("delta"):
                ok &= bar("%s <= zrl_encode_device" % name, ms <= zrl, ms, zrl)
                print("    %.0f GB/s moved (%d n)" % ((3 if "decode" in name else 2) * n / ms / 1e6, 3 if "decode" in name else 2))
        # sides that start off a 16-byte boundary (no bar)
        calls = [("delta_encode_device w=4, in + 1", lambda: ctx.delta_encode_device(x.ptr + 1, n - 16, 4, back)),
                 ("delta_encode_device w=4, out + 1", lambda: ctx.delta_encode_device(x, n - 16, 4, back.ptr + 1)),
                 ("delta_decode_device w=4, in + 1", lambda: ctx.delta_decode_device(x.ptr + 1, n - 16, 4, back)),
                 ("delta_decode_device w=4, out + 1", lambda: ctx.delta_decode_device(x, n - 16, 4, back.ptr + 1))]
        rounds(ctx, calls, 1)
        print("2^%d - 16 bytes, one side one byte off a 16-byte boundary (no bar): %d rounds" % (args.log2n, reps))
        report(rounds(ctx, calls, reps))
        # the segment form: segments of 64 KiB, widths cycling, every third one copied (no bar)
        count = max(n >> 16, 1)
        ls = [n // count] * count
        ws = [(1, 2, 4, 8)[k % 4] for k in range(count)]
        fs = [0 if k % 3 == 2 else 1 for k in range(count)]
        calls = [("delta_encode_segments_f_device", lambda: ctx.delta_encode_segments_f_device(x, ls, ws, fs, back)),
                 ("delta_decode_segments_f_device", lambda: ctx.delta_decode_segments_f_device(x, ls, ws, fs, back))]
        rounds(ctx, calls, 1)
        ctx.delta_encode_segments_f_device(x, ls, ws, fs, back)
        ctx.delta_decode_segments_f_device(back, ls, ws, fs, y)
        assert ctx.device_equal(y, x, n), "decode(encode(x)) != x, segments"
        print("%d segments of %d bytes, widths cycling 1, 2, 4, 8, every third one copied (no bar): %d rounds" % (count, ls[0], reps))
        report(rounds(ctx, calls, reps))
        for d in (x, y, r, back, f):
            d.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
