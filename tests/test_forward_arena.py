"""CPU suite: the arena of the narrow forward as plain arithmetic (bwts_debug_forward_arena: no context, no device).

The arena is one declared layout; what must hold whatever that layout is: it covers the four n-sized arrays no call can do without
(two u64 key buffers and two u32 value buffers: 24 n bytes), and it is no larger at any n than the hand-made sum it replaced.  The
old sum's values are recorded data (tests/golden/forward_arena_parent.json, taken from a build of the commit before the layout);
no formula of the engine is restated here."""
import ctypes
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_arena_parent.json")


def arena(pkg, n):
    out = (ctypes.c_uint64 * 1)()
    assert pkg.lib().bwts_debug_forward_arena(n, out) == 0, n
    return int(out[0])


def sizes():
    ns = set()
    for k in range(33):
        for d in (-1, 0, 1):
            n = (1 << k) + d
            if 1 <= n <= 1 << 32:
                ns.add(n)
    return sorted(ns)


def test_arena_holds_the_sort_buffers(pkg):
    for n in sizes():
        assert arena(pkg, n) >= 24 * n, n


def test_arena_never_grew(pkg):
    with open(FIXTURE) as f:
        parent = {int(n): int(b) for n, b in json.load(f)["bytes"].items()}
    assert sorted(parent) == sizes()
    for n in sizes():
        assert arena(pkg, n) <= parent[n], (n, arena(pkg, n), parent[n])


def test_bad_sizes_are_refused(pkg):
    out = (ctypes.c_uint64 * 1)()
    L = pkg.lib()
    assert L.bwts_debug_forward_arena(0, out) == -1
    assert L.bwts_debug_forward_arena((1 << 32) + 1, out) == -1


def test_no_wrap_at_2p32(pkg):
    assert arena(pkg, 1 << 32) > arena(pkg, 1 << 31)
