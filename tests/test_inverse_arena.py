"""CPU suite: the arena of the narrow inverse as plain arithmetic (bwts_debug_inverse_arena: no context, no device).

Two things must hold whatever the layout of the arena is.  The host path's helper thread allocates the arena before the transform
runs, from a hint: the hint must cover what the default attempt (moments, the splitter spacing the engine picks) then reserves, or
that allocation is thrown away.  And an attempt must reserve at least what its mark's arrays cannot do without: 4 n bytes of LF for
all of them, n more for the byte map, 4 n more for the index log.  Inequalities only: no formula of the engine is restated here."""
import ctypes

MARK_LOG, MARK_SENTINEL, MARK_BYTEMAP, MARK_MOMENTS = 0, 1, 2, 3


def arena(pkg, n, g, mark):
    out = (ctypes.c_uint64 * 2)()
    used = pkg.lib().bwts_debug_inverse_arena(n, g, mark, out)
    assert used >= 0, (n, g, mark)
    return int(out[0]), int(out[1]), used


def sizes():
    ns = set()
    for k in range(33):
        for d in (-1, 0, 1):
            n = (1 << k) + d
            if 1 <= n <= 1 << 32:
                ns.add(n)
    return sorted(ns)


def test_hint_covers_the_default_attempt(pkg):
    for n in sizes():
        request, hint, g = arena(pkg, n, -1, MARK_MOMENTS)
        assert 0 <= g <= 20, (n, g)
        assert hint >= request, (n, g, hint, request)
        # the hook's own g and an explicit one agree
        assert arena(pkg, n, g, MARK_MOMENTS)[0] == request, (n, g)


def test_every_mark_reserves_its_arrays(pkg):
    least = {MARK_MOMENTS: lambda n: 4 * n, MARK_SENTINEL: lambda n: 4 * n, MARK_BYTEMAP: lambda n: 5 * n, MARK_LOG: lambda n: 8 * n}
    for n in sizes():
        for mark, floor in least.items():
            request, _, g = arena(pkg, n, -1, mark)
            assert request >= floor(n), (n, g, mark, request)


def test_bad_arguments_are_refused(pkg):
    out = (ctypes.c_uint64 * 2)()
    L = pkg.lib()
    assert L.bwts_debug_inverse_arena(0, -1, MARK_MOMENTS, out) == -1
    assert L.bwts_debug_inverse_arena((1 << 32) + 1, -1, MARK_MOMENTS, out) == -1
    assert L.bwts_debug_inverse_arena(1 << 20, 21, MARK_MOMENTS, out) == -1
    assert L.bwts_debug_inverse_arena(1 << 20, -1, 4, out) == -1
