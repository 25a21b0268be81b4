"""GPU suite of the delta filter (include/bwts_delta.h): encode and decode byte for byte against the CPU model (tests/delta_model.py) at
every width and at every length where the kernels take another path, on full-range elements whose sums wrap and on all-0xFF inputs,
with both sides one byte off a 16-byte boundary and marks behind every output; one input whose tile sums take every level of the carry
scan; the segment form with mixed widths and filters and every start off alignment; the argument and range codes; the host forms."""
import numpy as np
import pytest

import delta_model as D
from test_planes_gpu import MARK, down, run_marked, some_bytes, up

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -5
# one tile more than one workgroup's carry scan takes (scan_templ.h: SCAN_SINGLE_BLOCK_MAX = 8192 tile sums), and a tail of five elements
DEEP = 8193 * 4096 + 5
# widths 1, 2, 4, 8 with filters 0 and 1; odd lengths, so that every start behind the first is off alignment; a full tile and more at
# every width; and a segment of all-0xFF elements (every sum an odd one out) directly in front of filtered ones: the carry must restart
SEG = [(4099, 1, 1), (8195, 2, 1), (33003, 1, 0), (16389, 4, 1), (32775, 8, 1), (4097, 4, 0), (65537, 8, 1), (5, 8, 1), (12289, 2, 1), (70001, 2, 0),
       (9, 4, 1), (4097, 1, 1)]
SEG_FF = (3, 6, 10)          # the segments that are all 0xFF: filtered, and directly in front of filtered segments


def sizes_for(w):
    T = D.E * w
    return [1, w - 1, w, w + 1, T - 1, T, T + 1, 2 * T + (w - 1)]


@pytest.fixture(scope="module")
def bufs(ctx):
    a, b, c = (ctx.alloc(sum(s[0] for s in SEG) + 512) for _ in range(3))
    yield a, b, c
    for d in (a, b, c):
        d.free()


@pytest.mark.parametrize("w", D.WIDTHS)
def test_encode_and_decode_against_the_model(pkg, ctx, bufs, w):
    a, b, c = bufs
    for n in sizes_for(w):
        if n == 0:
            continue
        for kind, x in (("random", some_bytes(n, n + w)), ("0xFF", np.full(n, 0xFF, dtype=np.uint8))):
            y = D.encode(x, w)
            for in_off, out_off in ((0, 0), (1, 1), (1, 0), (0, 15)):
                what = "%s w=%d n=%d in+%d out+%d" % (kind, w, n, in_off, out_off)
                run_marked(pkg, ctx, lambda s, d: ctx.delta_encode_device(s, n, w, d), a, n, in_off, b, out_off, x, y, "encode " + what)
                assert ctx.timings().n == n and ctx.timings().total_ms > 0
                run_marked(pkg, ctx, lambda s, d: ctx.delta_decode_device(s, n, w, d), b, n, in_off, c, out_off, y, x, "decode " + what)
            # the random bytes as a coded input: their sums wrap at every width
            run_marked(pkg, ctx, lambda s, d: ctx.delta_decode_device(s, n, w, d), a, n, 1, c, 1, x, D.decode(x, w), "decode of any bytes " + what)


def test_every_level_of_the_carry_scan(pkg, ctx):
    """Width 1, 8193 * 4096 + 5 bytes: 8194 tile sums, one more than one workgroup scans, so the scan of the sums runs its second
    level.  Full-range bytes: every tile's sum matters mod 256."""
    n = DEEP
    x = some_bytes(n, 77)
    a, b = ctx.alloc(n + 32), ctx.alloc(n + 96)
    try:
        up(pkg, ctx, a.ptr + 1, x)
        up(pkg, ctx, b.ptr + n, np.full(96, MARK, dtype=np.uint8))
        ctx.delta_decode_device(a.ptr + 1, n, 1, b.ptr + 1)
        got = down(pkg, ctx, b.ptr + 1, n + 64)
        assert (got[n:] == MARK).all()
        want = D.decode(x, 1)
        assert np.array_equal(got[:n], want), "decode: first difference at %d" % int(np.flatnonzero(got[:n] != want)[0])
        ctx.delta_encode_device(b.ptr + 1, n, 1, a.ptr + 1)
        assert np.array_equal(down(pkg, ctx, a.ptr + 1, n), x)
    finally:
        a.free()
        b.free()


def test_segments_mixed(pkg, ctx, bufs):
    a, b, c = bufs
    ls, ws, fs = [s[0] for s in SEG], [s[1] for s in SEG], [s[2] for s in SEG]
    starts = np.cumsum([0] + ls[:-1])
    n = sum(ls)
    x = some_bytes(n, 9)
    for k in SEG_FF:
        assert fs[k] == 1 and fs[k + 1] == 1
        x[starts[k]:starts[k] + ls[k]] = 0xFF
    y = D.encode_segments(x, ls, ws, fs)
    for in_off, out_off in ((5, 5), (0, 0), (7, 14)):
        assert all((in_off + int(s)) % 16 and (out_off + int(s)) % 16 for s in starts[1:])       # every start behind the first is off alignment, on both sides
        run_marked(pkg, ctx, lambda s, d: ctx.delta_encode_segments_f_device(s, ls, ws, fs, d), a, n, in_off, b, out_off, x, y, "encode segments")
        assert ctx.timings().n == n
        run_marked(pkg, ctx, lambda s, d: ctx.delta_decode_segments_f_device(s, ls, ws, fs, d), b, n, in_off, c, out_off, y, x, "decode segments")
        # any bytes as the coded side: the 0xFF segments make carries that the segments behind them must not see
        run_marked(pkg, ctx, lambda s, d: ctx.delta_decode_segments_f_device(s, ls, ws, fs, d), a, n, in_off, c, out_off, x, D.decode_segments(x, ls, ws, fs),
                   "decode segments of any bytes")
    # one segment is the single call; no filter anywhere is a copy; many equal segments
    run_marked(pkg, ctx, lambda s, d: ctx.delta_encode_segments_f_device(s, [n], [4], [1], d), a, n, 1, b, 0, x, D.encode(x, 4), "one segment")
    run_marked(pkg, ctx, lambda s, d: ctx.delta_decode_segments_f_device(s, ls, ws, [0] * len(ls), d), a, n, 1, b, 3, x, x, "no filter")
    many = [4097] * 50
    x = some_bytes(sum(many), 41)
    run_marked(pkg, ctx, lambda s, d: ctx.delta_decode_segments_f_device(s, many, [2] * 50, [1] * 50, d), a, x.size, 0, b, 0, x,
               D.decode_segments(x, many, [2] * 50, [1] * 50), "50 segments")


def test_errors(pkg, ctx, bufs):
    a, b, c = bufs
    L, h = pkg.lib(), ctx._h
    x = some_bytes(5000, 1)
    a.upload(x)
    kept = []

    def arr(*v, dtype=np.uint64):
        kept.append(np.array(v, dtype=dtype))       # (alive until the test ends)
        return kept[-1].ctypes.data

    def u32(*v):
        return arr(*v, dtype=np.uint32)

    for fn, seg in ((L.bwts_delta_encode_device, L.bwts_delta_encode_segments_f_device), (L.bwts_delta_decode_device, L.bwts_delta_decode_segments_f_device)):
        for w in (0, 3, 16, 5, 6, 7, 0x10004, 0x101):
            assert fn(h, a.ptr, 5000, w, b.ptr) == E_ARG, w
            assert seg(h, a.ptr, arr(3000, 2000), u32(4, w), u32(1, 1), 2, b.ptr) == E_ARG, w
            assert seg(h, a.ptr, arr(3000, 2000), u32(4, w), u32(1, 0), 2, b.ptr) == E_ARG, w      # a bad width is refused where it is copied too
        for f in (2, 3, 255, 0x100, 0xFFFFFFFF):
            assert seg(h, a.ptr, arr(3000, 2000), u32(4, 1), u32(0, f), 2, b.ptr) == E_ARG, f
        assert fn(None, a.ptr, 5000, 4, b.ptr) == E_ARG and fn(h, None, 5000, 4, b.ptr) == E_ARG and fn(h, a.ptr, 5000, 4, None) == E_ARG
        assert fn(h, a.ptr, 0, 4, b.ptr) == E_ARG
        assert fn(h, a.ptr, 1000, 4, a.ptr + 999) == E_ARG and fn(h, a.ptr, 1000, 4, a.ptr - 999) == E_ARG and fn(h, a.ptr, 1000, 4, a.ptr) == E_ARG        # overlap
        assert fn(h, a.ptr, 1000, 4, a.ptr + 1000) == 0
        assert fn(h, a.ptr, (1 << 36) + 1, 4, b.ptr) == E_RANGE
        assert seg(h, a.ptr, arr(3000, 0, 2000), u32(1, 2, 4), u32(1, 1, 1), 3, b.ptr) == E_ARG                 # a zero length
        assert seg(h, a.ptr, arr(3000, 2000), u32(1, 2), u32(1, 1), 0, b.ptr) == E_ARG and seg(h, a.ptr, None, u32(1, 2), u32(1, 1), 2, b.ptr) == E_ARG
        assert seg(h, a.ptr, arr(3000, 2000), None, u32(1, 1), 2, b.ptr) == E_ARG and seg(h, a.ptr, arr(3000, 2000), u32(1, 2), None, 2, b.ptr) == E_ARG
        assert seg(h, a.ptr, arr(600, 400), u32(1, 2), u32(1, 1), 2, a.ptr + 992) == E_ARG                       # overlap
        assert seg(h, a.ptr, arr(1 << 31, 1 << 31, 1), u32(1, 2, 4), u32(1, 1, 1), 3, b.ptr) == E_RANGE          # the lengths alone decide
    hp = np.zeros(64, dtype=np.uint8).ctypes.data
    for fn in (L.bwts_delta_encode, L.bwts_delta_decode):
        assert fn(h, hp, 64, 3, hp) == E_ARG and fn(h, hp, 0, 4, hp) == E_ARG and fn(h, None, 64, 4, hp) == E_ARG and fn(h, hp, (1 << 36) + 1, 4, hp) == E_RANGE
    # the context works afterwards (the adjacent call above wrote into a)
    a.upload(x)
    ctx.delta_encode_device(a, 5000, 4, b)
    assert np.array_equal(b.download(5000), D.encode(x, 4))


def test_host_forms(pkg, ctx):
    for w in D.WIDTHS:
        for n in (1, w + 1, 70001):
            x = some_bytes(n, 3 * n + w)
            y = ctx.delta_encode(x, w)
            assert np.array_equal(y, D.encode(x, w)), (w, n)
            assert np.array_equal(ctx.delta_decode(y, w), x), (w, n)
    with pytest.raises(pkg.BwtsError) as e:
        ctx.delta_encode(b"abcdefgh", 3)
    assert e.value.code == E_ARG
