"""GPU suite of the byte-plane split at a width per segment (include/bwts_members.h: bwts_planes_split_segments_w_device and its join):
byte for byte against the CPU model per segment (tests/pack_members_model.py over tests/planes_model.py) on the member set that
meets every boundary, with both base pointers on and off a 16-byte boundary and marks around every output; with all widths alike,
the bytes of the uniform segment call; widths of 1 alone (a copy through every tile path); the argument errors."""
import numpy as np
import pytest

import members_cases as C
import pack_members_model as MM
import planes_model as S
from test_planes_gpu import MARK, down, some_bytes, up

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -5
N = sum(C.LENGTHS)
FRONT = 48                      # marks in front of an output


@pytest.fixture(scope="module")
def bufs(ctx):
    a, b, c = (ctx.alloc(N + 512) for _ in range(3))
    yield a, b, c
    for d in (a, b, c):
        d.free()


@pytest.fixture(scope="module")
def reference():
    """The member set's bytes and their split at the set's widths: computed once, shared, left unchanged."""
    members, widths = C.member_set()
    x = np.frombuffer(b"".join(members), dtype=np.uint8)
    y = np.frombuffer(MM.split_segments(x.tobytes(), C.LENGTHS, widths), dtype=np.uint8)
    return x, y, widths


def run_marked(pkg, ctx, call, src, n, in_off, dst, out_off, x, want, what):
    """x at src + in_off; marks over dst, FRONT + out_off of them in front of the output and 64 behind; the call; dst again."""
    lead = FRONT + out_off
    up(pkg, ctx, src.ptr + in_off, x)
    up(pkg, ctx, dst.ptr, np.full(lead + n + 64, MARK, dtype=np.uint8))
    call(src.ptr + in_off, dst.ptr + lead)
    got = down(pkg, ctx, dst.ptr, lead + n + 64)
    assert (got[:lead] == MARK).all() and (got[lead + n:] == MARK).all(), "%s: a mark was overwritten" % what
    if not np.array_equal(got[lead:lead + n], want):
        bad = np.flatnonzero(got[lead:lead + n] != want)
        raise AssertionError("%s: %d bytes differ, the first at %d of %d" % (what, bad.size, int(bad[0]), n))


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (0, 1), (5, 11), (15, 9)])
def test_mixed_widths_against_the_model(pkg, ctx, bufs, reference, in_off, out_off):
    a, b, c = bufs
    x, y, widths = reference
    ls = C.LENGTHS
    what = "in+%d out+%d" % (in_off, out_off)
    run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_w_device(s, ls, widths, d), a, N, in_off, b, out_off, x, y, "split " + what)
    assert ctx.timings().n == N and ctx.timings().total_ms > 0
    run_marked(pkg, ctx, lambda s, d: ctx.planes_join_segments_w_device(s, ls, widths, d), b, N, in_off, c, out_off, y, x, "join " + what)
    assert ctx.timings().n == N


def test_every_width_meets_every_length(pkg, ctx, bufs, reference):
    """The widths rotated against the lengths: every length of the set at every width, all starts off alignment."""
    a, b, c = bufs
    x = reference[0]
    for shift in (1, 2, 3):
        widths = [(1, 2, 4, 8)[(k + shift) % 4] for k in range(len(C.LENGTHS))]
        y = np.frombuffer(MM.split_segments(x.tobytes(), C.LENGTHS, widths), dtype=np.uint8)
        run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_w_device(s, C.LENGTHS, widths, d), a, N, 3, b, 7, x, y, "split, widths rotated by %d" % shift)
        run_marked(pkg, ctx, lambda s, d: ctx.planes_join_segments_w_device(s, C.LENGTHS, widths, d), b, N, 7, c, 3, y, x, "join, widths rotated by %d" % shift)


@pytest.mark.parametrize("w", S.WIDTHS)
def test_all_widths_alike_is_the_uniform_call(pkg, ctx, bufs, reference, w):
    a, b, c = bufs
    x = reference[0]
    ls = C.LENGTHS
    up(pkg, ctx, a.ptr + 1, x)
    ctx.planes_split_segments_device(a.ptr + 1, ls, w, c.ptr + 2)
    uniform = down(pkg, ctx, c.ptr + 2, N)
    assert np.array_equal(uniform, S.split_segments(x, ls, w))
    run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_w_device(s, ls, [w] * len(ls), d), a, N, 1, b, 2, x, uniform, "split, all at %d" % w)
    run_marked(pkg, ctx, lambda s, d: ctx.planes_join_segments_w_device(s, ls, [w] * len(ls), d), b, N, 2, c, 1, uniform, x, "join, all at %d" % w)


def test_width_1_copies(pkg, ctx, bufs):
    """Segments of width 1 alone, around the copied tile's size: one byte, one tile less a byte, a tile, a tile and a byte, two and a tail."""
    a, b, c = bufs
    T = MM.COPY_T
    ls = [1, T - 1, T, T + 1, 2 * T + 17, 15, 16, 17]
    x = some_bytes(sum(ls), 7)
    for in_off, out_off in ((0, 0), (3, 9), (9, 3)):
        for call in (ctx.planes_split_segments_w_device, ctx.planes_join_segments_w_device):
            run_marked(pkg, ctx, lambda s, d: call(s, ls, [1] * len(ls), d), a, x.size, in_off, b, out_off, x, x, "copy in+%d out+%d" % (in_off, out_off))
    # one segment, at every width
    for w in (1, 2, 4, 8):
        n = 70001
        want = x[:n] if w == 1 else S.split(x[:n], w)
        run_marked(pkg, ctx, lambda s, d: ctx.planes_split_segments_w_device(s, [n], [w], d), a, n, 1, b, 0, x[:n], want, "one segment at %d" % w)


def test_errors(pkg, ctx, bufs):
    a, b, c = bufs
    L, h = pkg.lib(), ctx._h
    x = some_bytes(5000, 1)
    a.upload(x)
    kept = []

    def arr(*v, dtype=np.uint64):
        kept.append(np.array(v, dtype=dtype))       # (alive until the test ends)
        return kept[-1].ctypes.data

    def ws(*v):
        return arr(*v, dtype=np.uint32)

    for fn in (L.bwts_planes_split_segments_w_device, L.bwts_planes_join_segments_w_device):
        for w in (0, 3, 16, 5, 6, 7, 0x10004, 0x10001):
            assert fn(h, a.ptr, arr(3000, 2000), ws(4, w), 2, b.ptr) == E_ARG, w
        assert fn(h, a.ptr, arr(3000, 2000), None, 2, b.ptr) == E_ARG                               # widths == NULL
        assert fn(None, a.ptr, arr(3000, 2000), ws(4, 1), 2, b.ptr) == E_ARG and fn(h, None, arr(3000, 2000), ws(4, 1), 2, b.ptr) == E_ARG
        assert fn(h, a.ptr, arr(3000, 2000), ws(4, 1), 2, None) == E_ARG and fn(h, a.ptr, None, ws(4, 1), 2, b.ptr) == E_ARG
        assert fn(h, a.ptr, arr(3000, 0, 2000), ws(4, 1, 2), 3, b.ptr) == E_ARG                     # a zero length
        assert fn(h, a.ptr, arr(3000, 2000), ws(4, 1), 0, b.ptr) == E_ARG
        assert fn(h, a.ptr, arr(600, 400), ws(4, 1), 2, a.ptr + 992) == E_ARG                       # overlap
        assert fn(h, a.ptr, arr(1 << 31, 1 << 31, 1), ws(4, 1, 8), 3, b.ptr) == E_RANGE             # the lengths alone decide
    # the context works afterwards
    ctx.planes_split_segments_w_device(a, [3000, 2000], [4, 1], b)
    assert np.array_equal(b.download(5000), np.concatenate((S.split(x[:3000], 4), x[3000:])))
