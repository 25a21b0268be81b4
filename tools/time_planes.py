"""Manual timing (GPU box) of the byte-plane split beside the zero-run stage, and of pack / unpack with frames of version 3 beside
version 2, in one process, all times total_ms of the call: every call warmed up, then the calls alternated and the minimum of --reps
rounds each.  The bar, both sides from this run, no further margin; exit code 1 when it is missed:
  stage   on 2^30 bytes resident in HBM, planes_split_device and planes_join_device at each width cost no more than
          zrl_encode_device on the move-to-front ranks of the bench default zipf(2^30, seed 1).
For the record, with no bar: a plain device-to-device copy of the same bytes; packed size / n of the device's frames of versions 2 and
3 for typed inputs of 1 MiB (one block) beside bz2 -9, the rows that gain nothing included; pack_device and unpack_device of versions
2 and 3 on a float32 field of 2^30 bytes, in one block and in blocks of 1 MiB.
    python tools/time_planes.py [--log2n 30] [--reps 6] > profiles/planes_stage.txt"""
import argparse
import bz2
import os
import sys

import numpy as np
import torch        # before the engine's library, as in bench.py: the HIP runtime that torch loads is the one the process uses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from time_ec import report, rounds  # noqa: E402

STEP = 20.0 / 65536         # the field's step per value: the 65 536 values of the suite's field span [0, 20)


def bar(name, ok, a, b):
    print("  bar: %s: %s (%.3f vs %.3f)" % (name, "holds" if ok else "MISSED", a, b), flush=True)
    return ok


def field(first, count, rng, dtype="<f4"):
    """values first .. first + count of sin(x) + 0.3 sin(7.1 x) + 1e-3 noise, x = STEP * index"""
    x = STEP * np.arange(first, first + count, dtype=np.float64)
    return (np.sin(x) + 0.3 * np.sin(7.1 * x) + 1e-3 * rng.standard_normal(count)).astype(dtype)


def typed_inputs(nbytes):
    """(name, width, bytes): the rows of the size table, seeded"""
    rng = np.random.default_rng(1)
    g32 = (0.02 * rng.standard_normal(nbytes // 4)).astype("<f4")
    g16 = (0.02 * rng.standard_normal(nbytes // 2)).astype("<f4")
    return [("f32 smooth field", 4, field(0, nbytes // 4, rng).tobytes()),
            ("f64 smooth field", 8, field(0, nbytes // 8, rng, "<f8").tobytes()),
            ("i32 random walk, steps +-50", 4, np.cumsum(rng.integers(-50, 51, nbytes // 4)).astype("<i4").tobytes()),
            ("f32 gaussian weights", 4, g32.tobytes()),
            ("bf16 gaussian weights", 2, ((g16.view("<u4") + 0x8000) >> 16).astype("<u2").tobytes()),
            ("f16 gaussian weights", 2, g16.astype("<f2").tobytes()),
            ("u16 Poisson counts, mean 40", 2, rng.poisson(40.0, nbytes // 2).astype("<u2").tobytes())]


def size_table(ctx, pkg, x, f, back, nbytes):
    print("packed size / n, inputs of %d bytes in one block: the device's frames of version 2 (as it is) and version 3 (planes split first), and bz2 -9" % nbytes)
    print("  %-30s %5s %9s %9s %9s" % ("input (numpy, seeded)", "width", "version 2", "version 3", "bz2"))
    for name, w, data in typed_inputs(nbytes):
        n = len(data)
        x.upload(np.frombuffer(data, dtype=np.uint8))
        sizes = []
        for kw in ({"version": 2}, {"planes": w}):
            got = ctx.pack_device(x, n, 0, f, pkg.pack_bound(n, 0, **kw), **kw)
            assert ctx.unpack_device(f, got, back, n) == n and ctx.device_equal(back, x, n), (name, kw)
            sizes.append(got)
        print("  %-30s %5d %9.3f %9.3f %9.3f" % (name, w, sizes[0] / n, sizes[1] / n, len(bz2.compress(data, 9)) / n), flush=True)


def device_copy_ms(n, reps):
    """a plain device-to-device copy of n bytes, events around it: for orientation, not a bar"""
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    src.fill_(7)
    ms = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    del src, dst
    torch.cuda.empty_cache()
    return ms[1:]


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
        mib = min(n, 1 << 20)
        cap = max(pkg.pack_bound(n, mib, version=2), pkg.pack_bound(n, 0, version=2))
        x, y, r, back = (ctx.alloc(n) for _ in range(4))
        f, g = ctx.alloc(cap), ctx.alloc(cap)
        size = {}

        size_table(ctx, pkg, x, f, back, mib)

        # -- the stage beside the zero-run stage: 2^30 bytes resident, the seven calls alternated ---------------------------
        ctx.generate("zipf", 1, n, x)
        ctx.forward_device(x, n, y)
        ctx.mtf_forward_device(y, n, r)
        calls = [("zrl_encode_device (zipf ranks)", lambda: ctx.zrl_encode_device(r, n, y, n))]
        for w in (2, 4, 8):
            calls.append(("planes_split_device w=%d" % w, lambda w=w: ctx.planes_split_device(x, n, w, back)))
            calls.append(("planes_join_device w=%d" % w, lambda w=w: ctx.planes_join_device(x, n, w, back)))
        rounds(ctx, calls, 1)
        for w in (2, 4, 8):
            ctx.planes_split_device(x, n, w, back)
            ctx.planes_join_device(back, n, w, y)
            assert ctx.device_equal(y, x, n), "join(split(x)) != x at width %d" % w
        print("zipf 2^%d, seed 1 (the bench default): %d rounds, the seven calls alternated" % (args.log2n, reps))
        m = report(rounds(ctx, calls, reps))
        zrl = m["zrl_encode_device (zipf ranks)"]
        for name, ms in m.items():
            if name.startswith("planes"):
                ok &= bar("%s <= zrl_encode_device" % name, ms <= zrl, ms, zrl)
                print("    %.0f GB/s read + written" % (2 * n / ms / 1e6))
        # sides that start off a 16-byte boundary (no bar)
        calls = [("planes_split_device w=4, in + 1", lambda: ctx.planes_split_device(x.ptr + 1, n - 16, 4, back)),
                 ("planes_split_device w=4, out + 1", lambda: ctx.planes_split_device(x, n - 16, 4, back.ptr + 1)),
                 ("planes_join_device w=4, in + 1", lambda: ctx.planes_join_device(x.ptr + 1, n - 16, 4, back)),
                 ("planes_join_device w=4, out + 1", lambda: ctx.planes_join_device(x, n - 16, 4, back.ptr + 1))]
        rounds(ctx, calls, 1)
        print("2^%d - 16 bytes, one side one byte off a 16-byte boundary (no bar): %d rounds" % (args.log2n, reps))
        report(rounds(ctx, calls, reps))
        copy = device_copy_ms(n, reps)
        print("  plain device-to-device copy of 2^%d bytes (no bar): min %.3f ms (%s)" % (args.log2n, min(copy), " ".join("%.3f" % v for v in copy)), flush=True)

        # -- pack and unpack, version 3 beside version 2, on a float32 field -----------------------------------------------------
        rng = np.random.default_rng(2)
        piece = min(n // 4, 1 << 24)
        for first in range(0, n // 4, piece):
            part = field(first, piece, rng).view(np.uint8)
            ctx._check(pkg.lib().bwts_copy_to_device(ctx._h, x.ptr + 4 * first, part.ctypes.data, part.size))
        for what, m, b in (("one block", n, 0), ("blocks of 1 MiB", n, mib)):
            calls = [("pack_device v2", lambda: size.update(v2=ctx.pack_device(x, m, b, f, cap, version=2))),
                     ("pack_device v3 w=4", lambda: size.update(v3=ctx.pack_device(x, m, b, g, cap, planes=4))),
                     ("unpack_device v2", lambda: ctx.unpack_device(f, size["v2"], back, m)),
                     ("unpack_device v3 w=4", lambda: ctx.unpack_device(g, size["v3"], back, m))]
            rounds(ctx, calls, 1)
            assert ctx.device_equal(back, x, m), "unpack(pack(x)) != x"
            print("float32 field, %d bytes, %s (no bar): %d rounds, the four calls alternated" % (m, what, reps))
            report(rounds(ctx, calls, reps))
            print("  packed / n: version 2 %.4f, version 3 at width 4 %.4f" % (size["v2"] / m, size["v3"] / m), flush=True)
        for d in (x, y, r, back, f, g):
            d.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
