"""GPU suite (-m gpu): the input that used to end in "chunk table full" -- the byte planes at width 4 of a smooth float32 field of 2^29
bytes -- through the forward, the inverse and the packed frame.

The planes of such a field are deeply repetitive: half of their positions are tied after round 0, most of them in groups of more
than 2048 (the big list).  The chunks over the rest empty fast, the list is compacted and re-cut at the smallest nominal size, and
then tens of millions of elements leave the big list and are appended as chunks of that size: far more chunks than the first cut's
nominal size foresees.  While the chunk tables were sized by that first cut (a0 / S(a0) + 1024 entries) the forward answered
BWTS_E_INTERNAL here; they hold a0 / 2048 + 128 now, which is enough for every run (csrc/chunk_rounds.h, chunk_table_capacity;
tests/test_chunk_plan.py plays the worst run).  No CPU transform at this size: the round trip, checked on the device, and the engine's
report of its rounds are the check.  The arithmetic at test size is in tests/forward_cases.py (BWTS_CHUNK_TARGET)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 29
WIDTH = 4
STEP = 20.0 / 65536         # tools/time_planes.py: the field's step per value


def field_bytes(first, count, rng):
    """tools/time_planes.py field(): values first .. first + count of sin(x) + 0.3 sin(7.1 x) + 1e-3 noise as float32, x = STEP * index"""
    x = STEP * np.arange(first, first + count, dtype=np.float64)
    return (np.sin(x) + 0.3 * np.sin(7.1 * x) + 1e-3 * rng.standard_normal(count)).astype("<f4").view(np.uint8)


def test_planes_of_a_smooth_field_of_2p29_bytes(pkg):
    """field(0, 2^27, default_rng(1)) of tools/time_planes.py, made and uploaded in pieces of 2^24 values (one generator, so the draw is
    that of the single call).

    Wall time of the test on an MI355X machine: 4.4 s, of which 3.6 s make and upload the field and 0.7 s are device work."""
    t0 = time.time()
    rng = np.random.default_rng(1)
    piece = 1 << 24
    with pkg.Context(0) as ctx:
        x, planes, y, back = (ctx.alloc(N) for _ in range(4))
        cap = pkg.pack_bound(N, 0, planes=WIDTH)
        frame = ctx.alloc(cap)
        try:
            for first in range(0, N // 4, piece):
                part = field_bytes(first, piece, rng)
                ctx._check(pkg.lib().bwts_copy_to_device(ctx._h, x.ptr + 4 * first, part.ctypes.data, part.size))
            t1 = time.time()
            ctx.planes_split_device(x, N, WIDTH, planes)
            ctx.forward_device(planes, N, y)
            reps = ctx.debug_forward_report()
            ctx.inverse_device(y, N, back)
            assert ctx.device_equal(back, planes, N), "inverse(forward(planes)) != planes"

            for rep in reps:                    # (a suffix sort first when the factors were found by the general Lyndon path)
                print("report: %s" % {k: v for k, v in rep.items() if k != "round"})
                for r in rep["round"]:
                    print("  %s" % r)
                if rep["form"] == "chunks":
                    assert max(r["nchunks"] for r in rep["round"]) <= rep["chunks"]["maxchunks"] == rep["tied0"] // 2048 + 128, rep["chunks"]
                    assert rep["chunks"]["compactions_skipped"] == 0
            rep = reps[-1]
            assert rep["cyclic"] and rep["n"] == N and rep["form"] == "chunks", rep
            ch, a0 = rep["chunks"], rep["tied0"]
            assert ch["compactions"] >= 1 and ch["compactions_skipped"] == 0 and 0 < rep["chunk_S_recut"] < ch["S"], ch
            peak = max(r["nchunks"] for r in rep["round"])
            first_cut_capacity = a0 // ch["S"] + 1024                     # what the tables held while the first cut sized them
            print("a0 %d, S %d -> %d, chunks at most %d; capacity %d, sized by the first cut %d" %
                  (a0, ch["S"], rep["chunk_S_recut"], peak, ch["maxchunks"], first_cut_capacity))
            assert peak > first_cut_capacity, (peak, first_cut_capacity)
            assert peak <= ch["maxchunks"] == a0 // 2048 + 128, (peak, ch["maxchunks"])

            # the same field as one block of a version 3 frame
            got = ctx.pack_device(x, N, 0, frame, cap, planes=WIDTH)
            assert ctx.unpack_device(frame, got, back, N) == N
            assert ctx.device_equal(back, x, N), "unpack(pack(x)) != x"
            print("packed / n %.4f; host generation and upload %.1f s, device work %.1f s" % (got / N, t1 - t0, time.time() - t1))
        finally:
            for d in (x, planes, y, back, frame):
                d.free()
