"""GPU suite of the byte-plane split (include/bwts_planes.h): split and join byte for byte against the CPU model
(tests/planes_model.py) at every size where the kernels take another path, with both sides on and off a 16-byte boundary and marks
behind every output; the segment forms with every start off alignment; the argument errors; one input beyond 2^32 bytes; the host
forms; timings."""
import ctypes

import numpy as np
import pytest

import planes_model as S
from test_planes_model import SEGMENT_LENGTHS

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -5
TOP = (1 << 20) + 5
MARK = 0xA5


def sizes_for(w):
    T = S.E * w                                 # the tile: 4096 elements
    return [1, w - 1, w, w + 1, 16 * w - 1, 4095, 4097, T - 1, T, T + 1, 2 * T + w + 1, 70001, TOP]


def some_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.fixture(scope="module")
def bufs(ctx):
    a, b, c = (ctx.alloc(sum(SEGMENT_LENGTHS) + TOP + 256) for _ in range(3))
    yield a, b, c
    for d in (a, b, c):
        d.free()


def down(pkg, ctx, ptr, size):
    out = np.empty(size, dtype=np.uint8)
    ctx._check(pkg.lib().bwts_copy_to_host(ctx._h, out.ctypes.data, ptr, size))
    return out


def up(pkg, ctx, ptr, data):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    ctx._check(pkg.lib().bwts_copy_to_device(ctx._h, ptr, data.ctypes.data, data.size))


def run_marked(pkg, ctx, call, src, n, in_off, dst, out_off, x, want, what):
    """x at src + in_off, marks over dst, the call, and dst again: marks in front, the model's bytes, 64 marks behind."""
    up(pkg, ctx, src.ptr + in_off, x)
    up(pkg, ctx, dst.ptr, np.full(out_off + n + 64, MARK, dtype=np.uint8))
    call(src.ptr + in_off, dst.ptr + out_off)
    got = down(pkg, ctx, dst.ptr, out_off + n + 64)
    assert (got[:out_off] == MARK).all() and (got[out_off + n:] == MARK).all(), "%s: a mark was overwritten" % what
    if not np.array_equal(got[out_off:out_off + n], want):
        bad = np.flatnonzero(got[out_off:out_off + n] != want)
        raise AssertionError("%s: %d bytes differ, the first at %d of %d" % (what, bad.size, int(bad[0]), n))


@pytest.mark.parametrize("w", S.WIDTHS)
def test_split_and_join_against_the_model(pkg, ctx, bufs, w):
    a, b, c = bufs
    for n in sizes_for(w):
        x = some_bytes(n, n + w)
        y = S.split(x, w)
        assert pkg.debug_planes_plan(n, w) == S.plan(n, w)
        for in_off in (0, 1):
            for out_off in (0, 1):
                what = "w=%d n=%d in+%d out+%d" % (w, n, in_off, out_off)
                run_marked(pkg, ctx, lambda s, d: ctx.planes_split_device(s, n, w, d), a, n, in_off, b, out_off, x, y, "split " + what)
                assert ctx.timings().n == n and ctx.timings().total_ms > 0
                run_marked(pkg, ctx, lambda s, d: ctx.planes_join_device(s, n, w, d), b, n, in_off, c, out_off, y, x, "join " + what)


@pytest.mark.parametrize("w", S.WIDTHS)
def test_off_every_alignment(pkg, ctx, bufs, w):
    """One size of two tiles and a tail at every pair of offsets 0 .. 15 on one side, 3 on the other."""
    a, b, c = bufs
    n = 2 * S.E * w + 5 * w + (w - 1)
    x = some_bytes(n, w)
    y = S.split(x, w)
    for off in range(16):
        run_marked(pkg, ctx, lambda s, d: ctx.planes_split_device(s, n, w, d), a, n, off, b, 3, x, y, "split w=%d in+%d" % (w, off))
        run_marked(pkg, ctx, lambda s, d: ctx.planes_split_device(s, n, w, d), a, n, 3, b, off, x, y, "split w=%d out+%d" % (w, off))
        run_marked(pkg, ctx, lambda s, d: ctx.planes_join_device(s, n, w, d), b, n, off, c, 3, y, x, "join w=%d in+%d" % (w, off))
        run_marked(pkg, ctx, lambda s, d: ctx.planes_join_device(s, n, w, d), b, n, 3, c, off, y, x, "join w=%d out+%d" % (w, off))


@pytest.mark.parametrize("w", S.WIDTHS)
def test_segments(pkg, ctx, bufs, w):
    a, b, c = bufs
    ls = SEGMENT_LENGTHS
    starts = np.cumsum([0] + ls[:-1])
    n = sum(ls)
    x = some_bytes(n, 40 + w)
    y = S.split_segments(x, ls, w)
    for in_off, out_off in ((1, 1), (0, 0), (2, 9)):
        assert all((in_off + int(s)) % 16 and (out_off + int(s)) % 16 for s in starts[1:])       # every start behind the first is off alignment, on both sides
        run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_device(s, ls, w, d), a, n, in_off, b, out_off, x, y, "split segments w=%d" % w)
        assert ctx.timings().n == n
        run_marked(pkg, ctx, lambda s, d: ctx.planes_join_segments_device(s, ls, w, d), b, n, in_off, c, out_off, y, x, "join segments w=%d" % w)
    # one segment is the single call; many equal segments
    run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_device(s, [n], w, d), a, n, 1, b, 0, x, S.split(x, w), "one segment")
    many = [4097] * 50
    x = some_bytes(sum(many), 41)
    run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_device(s, many, w, d), a, x.size, 0, b, 0, x, S.split_segments(x, many, w), "50 segments")


def test_errors(pkg, ctx, bufs):
    a, b, c = bufs
    L, h = pkg.lib(), ctx._h
    x = some_bytes(5000, 1)
    a.upload(x)
    kept = []

    def arr(*v):
        kept.append(np.array(v, dtype=np.uint64))       # (alive until the test ends)
        return kept[-1].ctypes.data

    for fn, seg in ((L.bwts_planes_split_device, L.bwts_planes_split_segments_device), (L.bwts_planes_join_device, L.bwts_planes_join_segments_device)):
        for w in (0, 1, 3, 16, 5, 6, 7, 0x10004):
            assert fn(h, a.ptr, 5000, w, b.ptr) == E_ARG, w
            assert seg(h, a.ptr, arr(3000, 2000), 2, w, b.ptr) == E_ARG, w
        assert fn(None, a.ptr, 5000, 4, b.ptr) == E_ARG and fn(h, None, 5000, 4, b.ptr) == E_ARG and fn(h, a.ptr, 5000, 4, None) == E_ARG
        assert fn(h, a.ptr, 0, 4, b.ptr) == E_ARG
        assert fn(h, a.ptr, 1000, 4, a.ptr + 999) == E_ARG and fn(h, a.ptr, 1000, 4, a.ptr - 999) == E_ARG and fn(h, a.ptr, 1000, 4, a.ptr) == E_ARG        # overlap
        assert fn(h, a.ptr, 1000, 4, a.ptr + 1000) == 0
        assert fn(h, a.ptr, (1 << 36) + 1, 4, b.ptr) == E_RANGE
        assert seg(h, a.ptr, arr(3000, 0, 2000), 3, 4, b.ptr) == E_ARG                         # a zero length
        assert seg(h, a.ptr, arr(3000, 2000), 0, 4, b.ptr) == E_ARG and seg(h, a.ptr, None, 2, 4, b.ptr) == E_ARG
        assert seg(h, a.ptr, arr(600, 400), 2, 4, a.ptr + 992) == E_ARG                        # overlap
        assert seg(h, a.ptr, arr(1 << 31, 1 << 31, 1), 3, 4, b.ptr) == E_RANGE                 # the lengths alone decide
    hp = np.zeros(64, dtype=np.uint8).ctypes.data
    for fn in (L.bwts_planes_split, L.bwts_planes_join):
        assert fn(h, hp, 64, 3, hp) == E_ARG and fn(h, hp, 0, 4, hp) == E_ARG and fn(h, None, 64, 4, hp) == E_ARG and fn(h, hp, (1 << 36) + 1, 4, hp) == E_RANGE
    # the context works afterwards (the adjacent call above wrote into a)
    a.upload(x)
    ctx.planes_split_device(a, 5000, 4, b)
    assert np.array_equal(b.download(5000), S.split(x, 4))


def test_host_forms(pkg, ctx):
    for w in S.WIDTHS:
        for n in (1, w + 1, 70001):
            x = some_bytes(n, 3 * n + w)
            y = ctx.planes_split(x, w)
            assert np.array_equal(y, S.split(x, w)), (w, n)
            assert np.array_equal(ctx.planes_join(y, w), x), (w, n)
    with pytest.raises(pkg.BwtsError) as e:
        ctx.planes_split(b"abcdefgh", 3)
    assert e.value.code == E_ARG


def test_beyond_2p32(pkg, ctx):
    """n = 2^32 + 2^20 + 3 at width 4: join(split(x)) is x on the device, and three windows of the split against the model's
    definition over the input's own bytes: the first 4 KiB of plane 1, the bytes across offset 2^32, and the tail."""
    n, w = (1 << 32) + (1 << 20) + 3, 4
    q = n // w
    x, y, z = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    try:
        ctx.generate("zipf", 5, n, x)
        ctx.planes_split_device(x, n, w, y)
        assert ctx.timings().n == n
        ctx.planes_join_device(y, n, w, z)
        assert ctx.device_equal(z, x, n), "join(split(x)) != x"
        # plane 1, elements 0 .. 4095
        src = down(pkg, ctx, x.ptr, 4096 * w)
        assert np.array_equal(down(pkg, ctx, y.ptr + q, 4096), src[1::w])
        # the split's bytes [2^32 - 2048, 2^32 + 2048): they lie in plane 3
        lo = (1 << 32) - 2048
        k, i0 = divmod(lo, q)
        assert k == 3 and i0 + 4096 <= q
        src = down(pkg, ctx, x.ptr + i0 * w, 4096 * w)
        assert np.array_equal(down(pkg, ctx, y.ptr + lo, 4096), src[k::w])
        # the end of the last plane and the tail of 3 bytes
        src = down(pkg, ctx, x.ptr + n - 3 - 4096 * w, 4096 * w + 3)
        got = down(pkg, ctx, y.ptr + n - 3 - 4096, 4096 + 3)
        assert np.array_equal(got[:4096], src[3:4096 * w:w]) and np.array_equal(got[4096:], src[4096 * w:])
        assert src.any() and len(np.unique(src)) > 8
    finally:
        for d in (x, y, z):
            d.free()
