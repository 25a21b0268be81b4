"""CPU suite: the arena of one run of the forward beyond 2^32 as plain arithmetic (bwts_debug_wide_forward_arena: no context, no device).

The arena is one declared layout.  What must hold whatever that layout is: at no point of the grid is it larger than the hand-made sum
it replaced, and at every point it covers what no run can do without -- the rank array (8 n bytes; absent in the direct mode), a
bucket's two u64 key buffers, two u32 value buffers and four byte streams (28 bytes an element) and one segment's keys and output
bytes (9 bytes a position).  The old sum's values, and the bucket buffers' and the segment's sizes that go into the floor, are
recorded data (tests/golden/wide_forward_arena_parent.json, taken from a build of the commit before the layout); no formula of the
engine is restated here.

The grid: n at the corners of the rules that pick the bucket size, every mode (0 direct, 1 ranks, 2 suffix), the engine's own knobs
(seg_log2 = 0, bucket_cap = 0) and, at the two small n, the knobs of the forced runs in the GPU tests (segments of 2^13, buckets of n/6)."""
import ctypes
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_forward_arena_parent.json")
G = 1 << 30
SIZES = [1 << 12, (1 << 20) + 17, 1 << 30, (1 << 32) + 1, 12 * G, 13 * G + 1, 14 * G + 1, 24 * G, 48 * G + 1, 1 << 36]


def arena(pkg, n, mode, seg_log2=0, bucket_cap=0):
    out = (ctypes.c_uint64 * 1)()
    assert pkg.lib().bwts_debug_wide_forward_arena(n, mode, seg_log2, bucket_cap, out) == 0, (n, mode, seg_log2, bucket_cap)
    return int(out[0])


def grid():
    for n in SIZES:
        for mode in (0, 1, 2):
            yield n, mode, 0, 0
            if n < 1 << 30:
                yield n, mode, 13, max(256, n // 6)


def parent():
    with open(FIXTURE) as f:
        return {(p["n"], p["mode"], p["seg_log2"], p["bucket_cap"]): p for p in json.load(f)["points"]}


def test_fixture_covers_the_grid():
    assert sorted(parent()) == sorted(grid())


def test_arena_never_grew(pkg):
    old = parent()
    for point in grid():
        assert arena(pkg, *point) <= old[point]["bytes"], (point, arena(pkg, *point), old[point]["bytes"])


def test_arena_holds_what_every_run_needs(pkg):
    old = parent()
    for point in grid():
        n, mode = point[:2]
        floor = (8 * n if mode != 0 else 0) + 28 * old[point]["Mb"] + 9 * old[point]["seg"]
        assert arena(pkg, *point) >= floor, (point, arena(pkg, *point), floor)


def test_no_wrap_at_2p36(pkg):
    """(With its own knobs the direct mode picks a smaller bucket beyond 48 * 2^30 than below, and holds no n-sized array: there the two
    sizes are compared with the same bucket.)"""
    for mode in (1, 2):
        assert arena(pkg, 1 << 36, mode) > arena(pkg, 1 << 35, mode)
    for mode in (0, 1, 2):
        assert arena(pkg, 1 << 36, mode, 0, 1 << 30) > arena(pkg, 1 << 35, mode, 0, 1 << 30)


def test_bad_arguments_are_refused(pkg):
    out = (ctypes.c_uint64 * 1)()
    L = pkg.lib()
    assert L.bwts_debug_wide_forward_arena(0, 1, 0, 0, out) == -1
    assert L.bwts_debug_wide_forward_arena((1 << 36) + 1, 1, 0, 0, out) == -1
    assert L.bwts_debug_wide_forward_arena(1 << 20, -1, 0, 0, out) == -1
    assert L.bwts_debug_wide_forward_arena(1 << 20, 3, 0, 0, out) == -1
