"""GPU suite of the move-to-front stage (include/bwts_mtf.h): every case byte for byte against the CPU model (tests/mtf_model.py),
every forward result inverted on the device back to its input.  Sizes come from the engine's own plan (tile size T, tiles per
group G), so they sit on the tile ends, on the group boundary of the scan, and past two groups."""
import ctypes

import numpy as np
import pytest

import mtf_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -5


@pytest.fixture(scope="module")
def plan(pkg):
    p = pkg.debug_mtf_plan(1)
    return p["T"], p["G"]


@pytest.fixture(scope="module")
def bufs(ctx, plan):
    T, G = plan
    cap = max(2 * G * T + T + 7, 4096 * 3 * T, 3 * (8 << 20) + 1) + 64
    b = [ctx.alloc(cap) for _ in range(3)]
    yield b
    for d in b:
        d.free()


def _u8(x):
    return x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


def _model(fn_slow, fn_fast, x):
    x = _u8(x)
    return _u8(fn_slow(x.tobytes()) if x.size <= 20000 else fn_fast(x.tobytes()))


def _forward_checked(ctx, bufs, x):
    """mtf_forward_device of x == the model, and mtf_inverse_device of the result == x; returns the ranks."""
    x = _u8(x)
    a, b, c = bufs
    a.upload(x)
    ctx.mtf_forward_device(a, x.size, b)
    y = b.download(x.size)
    want = _model(M.forward, M.forward_fast, x)
    assert np.array_equal(y, want), "forward: first difference at %d of %d" % (int(np.flatnonzero(y != want)[0]), x.size)
    ctx.mtf_inverse_device(b, x.size, c)
    back = c.download(x.size)
    assert np.array_equal(back, x), "inverse of forward: first difference at %d of %d" % (int(np.flatnonzero(back != x)[0]), x.size)
    return y


def _inverse_checked(ctx, bufs, r):
    r = _u8(r)
    a, b, c = bufs
    a.upload(r)
    ctx.mtf_inverse_device(a, r.size, b)
    y = b.download(r.size)
    want = _model(M.inverse, M.inverse_fast, r)
    assert np.array_equal(y, want), "inverse: first difference at %d of %d" % (int(np.flatnonzero(y != want)[0]), r.size)
    ctx.mtf_forward_device(b, r.size, c)
    assert np.array_equal(c.download(r.size), r)


def _runs(rng, n):
    m = n // 40 + 2
    return np.repeat(rng.integers(0, 256, m, dtype=np.uint8), rng.integers(1, 131, m))[:n].copy()


def _cycle(n, down=False):
    base = np.arange(255, -1, -1, dtype=np.uint8) if down else np.arange(256, dtype=np.uint8)
    return np.resize(base, n)


def test_known_answers(ctx, bufs):
    assert _forward_checked(ctx, bufs, bytes([1, 1, 0, 2, 2, 1])).tolist() == [1, 0, 1, 2, 0, 2]
    y = _forward_checked(ctx, bufs, bytes(range(256)) * 2)
    assert y.tolist() == list(range(256)) + [255] * 256


def test_small_sizes_every_content(ctx, bufs, plan):
    T, _ = plan
    rng = np.random.default_rng(1)
    for n in (1, 2, 63, 64, 65, 127, 129, T - 1, T, T + 1, 2 * T + 1):
        _forward_checked(ctx, bufs, np.full(n, 0x5A, dtype=np.uint8))
        _forward_checked(ctx, bufs, _cycle(n))
        _forward_checked(ctx, bufs, _cycle(n, down=True))
        _forward_checked(ctx, bufs, rng.integers(0, 256, n, dtype=np.uint8))
        _forward_checked(ctx, bufs, _runs(rng, n))


def test_group_boundary_sizes(ctx, bufs, plan):
    """G*T - 1, G*T, G*T + 1: the last tile of the first group, and the first of the second."""
    T, G = plan
    rng = np.random.default_rng(2)
    _forward_checked(ctx, bufs, _runs(rng, G * T - 1))
    _forward_checked(ctx, bufs, np.full(G * T - 1, 3, dtype=np.uint8))
    _forward_checked(ctx, bufs, _cycle(G * T))
    _forward_checked(ctx, bufs, rng.integers(0, 256, G * T + 1, dtype=np.uint8))
    _forward_checked(ctx, bufs, _runs(rng, G * T + 1))


def test_more_than_one_group_state(ctx, bufs, plan):
    T, G = plan
    rng = np.random.default_rng(3)
    n = 2 * G * T + T + 7
    _forward_checked(ctx, bufs, _runs(rng, n))
    _forward_checked(ctx, bufs, np.full(n, 0xFF, dtype=np.uint8))


def test_late_first_occurrence(ctx, bufs, plan):
    """Tile 0 uses {7, 200}, tiles 1 and 2 other pairs; symbol 100 appears in the middle of tile 3 for the first time and again in
    tile G + 1: the carried order of the never-seen symbols and the union count d are wrong exactly here if compose is."""
    T, G = plan
    rng = np.random.default_rng(4)
    pairs = [(7, 200), (9, 3), (250, 1), (7, 3), (200, 31)]
    tiles = []
    for t in range(G + 3):
        m = T // 2
        tiles.append(np.repeat(rng.choice(np.array(pairs[t % len(pairs)], dtype=np.uint8), m), rng.integers(1, 9, m))[:T])
    x = np.concatenate(tiles)
    assert 100 not in x
    x[3 * T + T // 2] = 100
    x[(G + 1) * T + 5] = 100
    _forward_checked(ctx, bufs, x)
    _forward_checked(ctx, bufs, x[:4 * T + 1])


def test_second_stage_of_the_transform(ctx, bufs):
    """MTF of the device BWTS of the generators' zipf and text, against the model applied to the oracle's BWTS; then mtf_inverse_device
    and inverse_device give the input back."""
    a, b, c = bufs
    for kind, n in (("zipf", (1 << 20) + 1), ("text", 1 << 20)):
        x = _u8(O.generate(kind, n, 1))
        a.upload(x)
        ctx.forward_device(a, n, b)
        ctx.mtf_forward_device(b, n, c)
        want = _u8(M.forward_fast(_u8(O.forward(x)).tobytes()))
        assert np.array_equal(c.download(n), want), kind
        ctx.mtf_inverse_device(c, n, b)
        ctx.inverse_device(b, n, a)
        assert np.array_equal(a.download(n), x), kind


def test_inverse_of_any_bytes(ctx, bufs, plan):
    T, G = plan
    rng = np.random.default_rng(6)
    for n in (1, 65, T + 1, 2 * T + 1):
        _inverse_checked(ctx, bufs, rng.integers(0, 256, n, dtype=np.uint8))
        _inverse_checked(ctx, bufs, np.full(n, 255, dtype=np.uint8))
        _inverse_checked(ctx, bufs, np.zeros(n, dtype=np.uint8))
    _inverse_checked(ctx, bufs, rng.integers(0, 256, G * T + 1, dtype=np.uint8))
    _inverse_checked(ctx, bufs, np.zeros(G * T + 1, dtype=np.uint8))


def _segments_checked(ctx, bufs, x, lengths, singles=True):
    x = _u8(x)
    ls = np.asarray(lengths, dtype=np.uint64)
    n = int(ls.sum())
    assert n == x.size
    a, b, c = bufs
    a.upload(x)
    ctx.mtf_forward_segments_device(a, ls, b)
    y = b.download(n)
    fast = n > 20000
    want = _u8(M.segmented(M.forward_fast if fast else M.forward, x.tobytes(), ls))
    assert np.array_equal(y, want), "forward: first difference at %d" % int(np.flatnonzero(y != want)[0])
    ctx.mtf_inverse_segments_device(b, ls, c)
    assert np.array_equal(c.download(n), x)
    # ranks need not come from a forward: the input itself as ranks
    ctx.mtf_inverse_segments_device(a, ls, c)
    want_i = _u8(M.segmented(M.inverse_fast if fast else M.inverse, x.tobytes(), ls))
    assert np.array_equal(c.download(n), want_i)
    if singles:       # each segment equals the single call on that segment, both directions
        off = 0
        for ln in ls.tolist():
            ctx.mtf_forward_device(a.ptr + off, ln, c.ptr + off)
            off += ln
        assert np.array_equal(c.download(n), y)
        off = 0
        for ln in ls.tolist():
            ctx.mtf_inverse_device(a.ptr + off, ln, c.ptr + off)
            off += ln
        assert np.array_equal(c.download(n), want_i)


def test_segments(ctx, bufs, plan):
    T, G = plan
    rng = np.random.default_rng(7)
    for lengths in ([1], [1, 1, 1], [1] * 1000, [T - 1, 1, T + 1], [T, T, T]):
        n = sum(lengths)
        _segments_checked(ctx, bufs, rng.integers(0, 256, n, dtype=np.uint8), lengths)
        _segments_checked(ctx, bufs, _runs(rng, n), lengths, singles=False)
    lengths = [3 * T + 5, 2, G * T + 1, 7]
    _segments_checked(ctx, bufs, _runs(rng, sum(lengths)), lengths)
    x = rng.integers(0, 4, sum(lengths), dtype=np.uint8) + 40
    _segments_checked(ctx, bufs, x, lengths, singles=False)


def test_segments_4096_random_lengths(ctx, bufs, plan):
    T, _ = plan
    rng = np.random.default_rng(8)
    lengths = rng.integers(1, 3 * T + 1, 4096)
    _segments_checked(ctx, bufs, _runs(rng, int(lengths.sum())), lengths, singles=False)


def test_one_segment_equals_single_call(ctx, bufs, plan):
    T, _ = plan
    rng = np.random.default_rng(9)
    x = rng.integers(0, 256, 5 * T + 3, dtype=np.uint8)
    y = _forward_checked(ctx, bufs, x)
    a, b, _ = bufs
    a.upload(x)
    ctx.mtf_forward_segments_device(a, [x.size], b)
    assert np.array_equal(b.download(x.size), y)
    ctx.mtf_inverse_segments_device(b, [x.size], a)
    assert np.array_equal(a.download(x.size), x)


def test_errors(pkg, ctx, bufs):
    L = pkg.lib()
    a, b, _ = bufs
    one = (ctypes.c_uint64 * 1)(5)
    zero = (ctypes.c_uint64 * 3)(5, 0, 5)
    host = np.zeros(16, dtype=np.uint8)
    hp = host.ctypes.data
    for name in ("bwts_mtf_forward_device", "bwts_mtf_inverse_device"):
        fn = getattr(L, name)
        assert fn(ctx._h, None, 5, b.ptr) == E_ARG and fn(ctx._h, a.ptr, 5, None) == E_ARG and fn(None, a.ptr, 5, b.ptr) == E_ARG
        assert fn(ctx._h, a.ptr, 0, b.ptr) == E_ARG
        assert fn(ctx._h, a.ptr, 1000, a.ptr + 999) == E_ARG and fn(ctx._h, a.ptr + 10, 1000, a.ptr) == E_ARG     # overlap
        assert fn(ctx._h, a.ptr, (1 << 36) + 1, b.ptr) == E_RANGE
    for name in ("bwts_mtf_forward", "bwts_mtf_inverse"):
        fn = getattr(L, name)
        assert fn(ctx._h, None, 5, hp) == E_ARG and fn(ctx._h, hp, 5, None) == E_ARG and fn(ctx._h, hp, 0, hp) == E_ARG
    big = (ctypes.c_uint64 * 3)(1 << 31, 1 << 31, 1)
    for name, p, q in (("bwts_mtf_forward_segments_device", a.ptr, b.ptr), ("bwts_mtf_inverse_segments_device", a.ptr, b.ptr),
                       ("bwts_mtf_forward_segments", hp, hp), ("bwts_mtf_inverse_segments", hp, hp)):
        fn = getattr(L, name)
        assert fn(ctx._h, None, one, 1, q) == E_ARG and fn(ctx._h, p, one, 1, None) == E_ARG and fn(ctx._h, p, None, 1, q) == E_ARG
        assert fn(ctx._h, p, one, 0, q) == E_ARG
        assert fn(ctx._h, p, zero, 3, q) == E_ARG
        assert fn(ctx._h, p, big, 3, q) == E_RANGE          # the lengths alone decide: the data is not touched
    ten = (ctypes.c_uint64 * 2)(600, 400)
    assert L.bwts_mtf_forward_segments_device(ctx._h, a.ptr, ten, 2, a.ptr + 999) == E_ARG
    assert not host.any()


def test_host_forms(pkg, ctx, bufs):
    """Host buffers, more than one staging chunk, out == in; the bytes are those of the device form."""
    L = pkg.lib()
    rng = np.random.default_rng(10)
    n = 3 * (8 << 20) + 1
    x = _runs(rng, n)
    x[::4099] = rng.integers(0, 256, x[::4099].size, dtype=np.uint8)
    a, b, _ = bufs
    a.upload(x)
    ctx.mtf_forward_device(a, n, b)
    y_dev = b.download(n)
    y = ctx.mtf_forward(x)
    assert np.array_equal(y, y_dev)
    assert ctx.timings().n == n and ctx.timings().h2d_ms > 0
    buf = y.copy()
    assert L.bwts_mtf_inverse(ctx._h, buf.ctypes.data, n, buf.ctypes.data) == 0       # out == in
    assert np.array_equal(buf, x)
    lengths = np.array([n // 3, 1, n - n // 3 - 1], dtype=np.uint64)
    ys = ctx.mtf_forward_segments(x, lengths)
    ctx.mtf_forward_segments_device(a, lengths, b)
    assert np.array_equal(ys, b.download(n))
    assert np.array_equal(ys[:n // 3], y[:n // 3]) and ys[n // 3] == x[n // 3]
    back = ctx.mtf_inverse_segments(ys, lengths, out=ys)                                # out == in
    assert back is ys and np.array_equal(ys, x)
    small = rng.integers(0, 256, 1000, dtype=np.uint8)
    assert np.array_equal(ctx.mtf_inverse(ctx.mtf_forward(small)), small)
    assert ctx.mtf_forward(small).tobytes() == M.forward(small.tobytes())


def test_timings(ctx, bufs, plan):
    T, G = plan
    a, b, c = bufs
    for n in (5, 3 * T + 1):
        a.upload(np.arange(n, dtype=np.uint64).astype(np.uint8))
        for call, src, dst in ((ctx.mtf_forward_device, a, b), (ctx.mtf_inverse_device, b, c)):
            call(src, n, dst)
            t = ctx.timings()
            k = t.as_dict()["kernels"]
            assert t.n == n and t.total_ms > 0
            assert set(k) == {"other"} and k["other"]["launches"] == (1 if n <= T else 5)
    # the segmented forms build their tile table on the device: a sixth launch under the same class; and with every launch timed
    # the per-launch split (debug_last_spans) has one entry per launch
    n = 3 * T + 1
    ls = [T + 1, 2 * T]
    ctx.set_timing(2)
    try:
        for call, src, dst in ((ctx.mtf_forward_segments_device, a, b), (ctx.mtf_inverse_segments_device, b, c)):
            call(src, ls, dst)
            t = ctx.timings()
            k = t.as_dict()["kernels"]
            assert t.n == n and t.total_ms > 0 and set(k) == {"other"} and k["other"]["launches"] == 6
            spans = ctx.debug_last_spans()
            assert len(spans) == 6 and all(ms >= 0 for ms in spans)
            assert abs(sum(spans) - k["other"]["ms"]) < 1e-3
    finally:
        ctx.set_timing(0)
    ctx.mtf_forward_device(a, n, b)
    assert ctx.debug_last_spans() == []                      # timing off: no launch is timed
