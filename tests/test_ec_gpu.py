"""GPU suite of the entropy coder (include/bwts_ec.h): every stream byte for byte against the CPU model (tests/ec_model.py), every
stream decoded on the device back to its input, the model's own streams decoded on the device, the capacity contract, the segment
forms, malformed streams (each refused by the model first), the host forms, the error table and the timings.  Sizes come from the
engine's own plan (tile size T, tiles per block K): the tile ends, the block boundary, and past two blocks."""
import ctypes

import numpy as np
import pytest

import ec_model as E
import mtf_model as M
import oracle_lib as O
from test_ec_model import contents, malformed_cases, malformed_input

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE = -1, -5, -8, -9


@pytest.fixture(scope="module")
def plan(pkg):
    p = pkg.debug_ec_plan(1)
    assert (p["T"], p["K"]) == (E.T, E.K)
    return p["T"], p["K"]


@pytest.fixture(scope="module")
def bufs(pkg, ctx, plan):
    """a, c: byte side; b: coded side, as large as the bound of the largest input"""
    T, K = plan
    cap = max(2 * K * T + T + 7, 4096 * 3 * T, 3 * (8 << 20) + 1) + 64
    a, c = ctx.alloc(cap), ctx.alloc(cap)
    b = ctx.alloc(pkg.ec_bound(cap) + 4096 * 1024)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def _u8(x):
    return x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


def _first_diff(y, want):
    if y.size != want.size:
        return "sizes %d and %d" % (y.size, want.size)
    return "first difference at %d of %d" % (int(np.flatnonzero(y != want)[0]), y.size)


def _checked(pkg, ctx, bufs, x, capacity=True):
    """The five checks of one input: device stream == model stream, device decode of both == x, exact capacity, capacity - 16."""
    x = _u8(x)
    n = x.size
    a, b, c = bufs
    want = _u8(E.encode(x))
    a.upload(x)
    size = ctx.ec_encode_device(a, n, b, pkg.ec_bound(n))
    assert size == want.size, (n, size, want.size)
    y = b.download(size)
    assert np.array_equal(y, want), "encode n=%d: %s" % (n, _first_diff(y, want))
    assert ctx.ec_decode_device(b, size, c, n) == n
    back = c.download(n)
    assert np.array_equal(back, x), "decode n=%d: %s" % (n, _first_diff(back, x))
    b.upload(want)                                          # the model's stream, not the device's
    c.upload(np.zeros(n, dtype=np.uint8) if x.any() else np.ones(n, dtype=np.uint8))
    assert ctx.ec_decode_device(b, want.size, c, n + 5) == n
    assert np.array_equal(c.download(n), x)
    if capacity:
        mark = np.full(size + 64, 0xA5, dtype=np.uint8)
        b.upload(mark)
        assert ctx.ec_encode_device(a, n, b, size) == size                     # exact capacity
        assert np.array_equal(b.download(size + 64), np.concatenate((want, mark[size:])))
        b.upload(mark)
        got = ctypes.c_uint64(0)
        rc = pkg.lib().bwts_ec_encode_device(ctx._h, a.ptr, n, b.ptr, size - 16, ctypes.byref(got))
        assert rc == E_SPACE, (n, rc)
        assert np.array_equal(b.download(size + 64)[size - 16:], mark[size - 16:])      # nothing beyond out_cap
    return want


def _sizes(plan):
    T, K = plan
    return [1, 2, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, K * T - 1, K * T, K * T + 1, 2 * K * T + T + 7]


def test_known_answers(pkg, ctx, bufs):
    assert len(_checked(pkg, ctx, bufs, b"A")) == 800
    s = _checked(pkg, ctx, bufs, bytes([0, 0, 1, 0]))
    assert s[16 + 512 + 16:16 + 512 + 20].view("<u4")[0] == 623616


@pytest.mark.parametrize("name", ["repeat", "uniform", "geometric", "zeros98", "rare180", "two_1e5"])
def test_every_size(pkg, ctx, bufs, plan, name):
    for n in _sizes(plan):
        _checked(pkg, ctx, bufs, contents(n, n % 97)[name])


def test_rare_symbol_blocks_run_the_minus_loop(plan):
    """What makes rare180 the d < 0 case: in a full block the rule overshoots 4096 by more than any rare symbol's frequency."""
    T, K = plan
    x = contents(K * T, 0)["rare180"]
    h = np.bincount(x, minlength=256)
    first = np.where(h > 0, np.maximum(1, h * 4096 // h.sum()), 0)
    assert int(first.sum()) - 4096 > int(first[1:].max())


def test_third_stage_of_the_pipeline(pkg, ctx, bufs):
    """forward_device -> mtf_forward_device -> ec_encode_device against the model applied to the oracle's BWTS and the MTF model; then
    decode -> mtf_inverse_device -> inverse_device give the input back."""
    a, b, c = bufs
    for kind, n in (("zipf", (1 << 20) + 1), ("text", 1 << 20)):
        x = _u8(O.generate(kind, n, 1))
        a.upload(x)
        ctx.forward_device(a, n, c)
        ctx.mtf_forward_device(c, n, a)
        size = ctx.ec_encode_device(a, n, b, pkg.ec_bound(n))
        want = _u8(E.encode(_u8(M.forward_fast(_u8(O.forward(x)).tobytes()))))
        assert size == want.size and np.array_equal(b.download(size), want), kind
        assert size < n, kind
        assert ctx.ec_decode_device(b, size, c, n) == n
        ctx.mtf_inverse_device(c, n, a)
        ctx.inverse_device(a, n, c)
        assert np.array_equal(c.download(n), x), kind


def _segments_checked(pkg, ctx, bufs, x, lengths, singles):
    x = _u8(x)
    ls = np.asarray(lengths, dtype=np.uint64)
    n = int(ls.sum())
    assert n == x.size
    a, b, c = bufs
    want = E.encode_segments(x, ls.tolist())
    want_sizes = np.array([len(s) for s in want], dtype=np.uint64)
    total = int(want_sizes.sum())
    a.upload(x)
    sizes = ctx.ec_encode_segments_device(a, ls, b, pkg.ec_bound_segments(ls))
    assert np.array_equal(sizes, want_sizes)
    y = b.download(total)
    wcat = _u8(b"".join(want))
    assert np.array_equal(y, wcat), "segments: %s" % _first_diff(y, wcat)
    ctx.ec_decode_segments_device(b, sizes, ls, c)
    assert np.array_equal(c.download(n), x)
    # each stream equals the single call on that segment (singles: every segment, or every k-th), both directions
    offs = np.concatenate(([0], np.cumsum(ls))).astype(np.int64)
    soffs = np.concatenate(([0], np.cumsum(want_sizes))).astype(np.int64)
    for i in range(0, ls.size, singles):
        off, soff, ln, sz = int(offs[i]), int(soffs[i]), int(ls[i]), int(want_sizes[i])
        got = ctx.ec_encode_device(a.ptr + off, ln, c, pkg.ec_bound(ln))
        assert got == sz and np.array_equal(c.download(sz), y[soff:soff + sz]), i
        assert ctx.ec_decode_device(b.ptr + soff, sz, c, ln) == ln
        assert np.array_equal(c.download(ln), x[off:off + ln]), i
    # exact capacity, and 16 less
    got = ctx.ec_encode_segments_device(a, ls, b, total)
    assert np.array_equal(got, want_sizes)
    out = np.zeros(ls.size, dtype=np.uint64)
    rc = pkg.lib().bwts_ec_encode_segments_device(ctx._h, a.ptr, ls.ctypes.data, ls.size, b.ptr, total - 16, out.ctypes.data)
    assert rc == E_SPACE
    return sizes


def _ranks(rng, n):
    return np.minimum(rng.geometric(0.3, n) - 1, 255).astype(np.uint8)


def test_segments(pkg, ctx, bufs, plan):
    T, K = plan
    rng = np.random.default_rng(7)
    for lengths in ([1], [1] * 1000, [T - 1, 1, T + 1], [3 * T + 5, 2, K * T + 1, 7]):
        n = sum(lengths)
        _segments_checked(pkg, ctx, bufs, _ranks(rng, n), lengths, singles=1)
        _segments_checked(pkg, ctx, bufs, rng.integers(0, 256, n, dtype=np.uint8), lengths, singles=1)


def test_segments_4096_random_lengths(pkg, ctx, bufs, plan):
    """Every stream against the model's stream of that segment alone, and every eighth segment (512 of them) also against the
    device's single call on it."""
    T, _ = plan
    rng = np.random.default_rng(8)
    lengths = rng.integers(1, 3 * T + 1, 4096)
    _segments_checked(pkg, ctx, bufs, _ranks(rng, int(lengths.sum())), lengths, singles=8)


def test_segments_wrong_length_is_a_format_error(pkg, ctx, bufs, plan):
    T, _ = plan
    rng = np.random.default_rng(9)
    lengths = [T - 1, 1, T + 1]
    x = _ranks(rng, sum(lengths))
    a, b, c = bufs
    a.upload(x)
    sizes = ctx.ec_encode_segments_device(a, lengths, b, pkg.ec_bound_segments(lengths))
    for wrong in ([T - 1, 2, T + 1], [T - 2, 1, T + 1], [T - 1, 1, T]):
        assert E.decode_segments(b.download(int(sizes.sum())).tobytes(), sizes.tolist(), wrong) is None
        with pytest.raises(pkg.BwtsError) as e:
            ctx.ec_decode_segments_device(b, sizes, wrong, c)
        assert e.value.code == E_FORMAT, wrong
    ctx.ec_decode_segments_device(b, sizes, lengths, c)
    assert np.array_equal(c.download(x.size), x)


def test_malformed_streams(pkg, ctx, bufs):
    L = pkg.lib()
    a, b, c = bufs
    x = malformed_input()
    good, cases = malformed_cases(x)
    got = ctypes.c_uint64(0)

    def good_decodes():
        b.upload(_u8(good))
        c.upload(np.full(x.size, 0xEE, dtype=np.uint8))
        assert ctx.ec_decode_device(b, len(good), c, x.size) == x.size
        assert np.array_equal(c.download(x.size), x)

    good_decodes()
    for name, bad in cases:
        assert E.decode(bad) is None, name                       # the model refuses it first
        b.upload(_u8(bad + bytes(64)))
        rc = L.bwts_ec_decode_device(ctx._h, b.ptr, len(bad), c.ptr, x.size, ctypes.byref(got))
        assert rc == E_FORMAT, (name, rc)
        good_decodes()
    # a good stream into too little room
    b.upload(_u8(good))
    assert L.bwts_ec_decode_device(ctx._h, b.ptr, len(good), c.ptr, x.size - 1, ctypes.byref(got)) == E_SPACE
    good_decodes()


def _runs(rng, n):
    m = n // 40 + 2
    return np.repeat(rng.integers(0, 256, m, dtype=np.uint8), rng.integers(1, 131, m))[:n].copy()


def test_host_forms(pkg, ctx, bufs):
    """Host buffers, more than one staging chunk; the bytes are those of the device form; a failed call leaves out untouched."""
    L = pkg.lib()
    rng = np.random.default_rng(10)
    n = 3 * (8 << 20) + 1
    x = _runs(rng, n)
    a, b, c = bufs
    a.upload(x)
    size = ctx.ec_encode_device(a, n, b, pkg.ec_bound(n))
    s_dev = b.download(size)
    s = ctx.ec_encode(x)
    assert np.array_equal(s, s_dev)
    assert ctx.timings().n == n and ctx.timings().h2d_ms > 0
    assert np.array_equal(ctx.ec_decode(s), x)
    assert ctx.timings().n == n
    assert np.array_equal(ctx.ec_encode(x, out_cap=size), s)                       # exact capacity
    got = ctypes.c_uint64(77)
    out = np.full(size + 16, 0x3C, dtype=np.uint8)
    assert L.bwts_ec_encode(ctx._h, x.ctypes.data, n, out.ctypes.data, size - 16, ctypes.byref(got)) == E_SPACE
    assert (out == 0x3C).all() and got.value == 77
    out = np.full(n, 0x3C, dtype=np.uint8)
    assert L.bwts_ec_decode(ctx._h, s.ctypes.data, size, out.ctypes.data, n - 1, ctypes.byref(got)) == E_SPACE
    assert (out == 0x3C).all() and got.value == 77
    small = rng.integers(0, 4, 3 * E.T + 9, dtype=np.uint8)
    bad = ctx.ec_encode(small)
    bad[bad.size - 300] ^= 0x40                                                     # inside the last payload: found only by decoding
    assert E.decode(bad.tobytes()) is None
    assert L.bwts_ec_decode(ctx._h, bad.ctypes.data, bad.size, out.ctypes.data, n, ctypes.byref(got)) == E_FORMAT
    assert (out == 0x3C).all() and got.value == 77
    assert ctx.ec_encode(small).tobytes() == E.encode(small)
    assert np.array_equal(ctx.ec_decode(ctx.ec_encode(small)), small)


def test_errors(pkg, ctx, bufs):
    L = pkg.lib()
    a, b, c = bufs
    got = ctypes.c_uint64(0)
    g = ctypes.byref(got)
    h = ctx._h
    enc, dec = L.bwts_ec_encode_device, L.bwts_ec_decode_device
    a.upload(np.zeros(4096, dtype=np.uint8))
    size = ctx.ec_encode_device(a, 1000, b, 1 << 20)
    for fn, src, n, dst, cap in ((enc, a.ptr, 1000, b.ptr, 1 << 20), (dec, b.ptr, size, c.ptr, 1000)):
        assert fn(None, src, n, dst, cap, g) == E_ARG and fn(h, None, n, dst, cap, g) == E_ARG and fn(h, src, n, None, cap, g) == E_ARG
        assert fn(h, src, n, dst, cap, None) == E_ARG and fn(h, src, 0, dst, cap, g) == E_ARG
        assert fn(h, src, n, src + n - 1, cap, g) == E_ARG                                   # overlap
    assert enc(h, a.ptr, 1000, a.ptr - 1600, 1 << 20, g) == E_ARG                            # ... from below, through out_cap
    assert enc(h, a.ptr, 1000, b.ptr + 8, 1 << 20, g) == E_ARG and dec(h, b.ptr + 8, size, c.ptr, 1000, g) == E_ARG     # coded side: 16-byte aligned
    assert enc(h, a.ptr, 1000, a.ptr + 992, (1 << 64) - 1, g) == E_ARG and enc(h, a.ptr, 1000, a.ptr - 1600, (1 << 64) - 1, g) == E_ARG     # ... no wrap
    assert enc(h, a.ptr, (1 << 36) + 1, b.ptr, 1 << 20, g) == E_RANGE
    assert dec(h, b.ptr, pkg.ec_bound(1 << 36) + 16, c.ptr, 1000, g) == E_RANGE
    host = np.zeros(4096, dtype=np.uint8)
    hp = host.ctypes.data
    for fn in (L.bwts_ec_encode, L.bwts_ec_decode):
        assert fn(h, None, 16, hp, 4096, g) == E_ARG and fn(h, hp, 16, None, 4096, g) == E_ARG and fn(h, hp, 0, hp, 4096, g) == E_ARG
        assert fn(h, hp, 16, hp, 4096, None) == E_ARG and fn(None, hp, 16, hp, 4096, g) == E_ARG
    assert L.bwts_ec_encode(h, hp, (1 << 36) + 1, hp, 4096, g) == E_RANGE
    arr = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    one, zero, big, sb = arr(5), arr(5, 0, 5), arr(1 << 31, 1 << 31, 1), arr(800, 800, 800)
    out3 = arr(0, 0, 0)
    es, ds = L.bwts_ec_encode_segments_device, L.bwts_ec_decode_segments_device
    assert es(h, None, one, 1, b.ptr, 1 << 20, out3) == E_ARG and es(h, a.ptr, one, 1, None, 1 << 20, out3) == E_ARG
    assert es(h, a.ptr, None, 1, b.ptr, 1 << 20, out3) == E_ARG and es(h, a.ptr, one, 1, b.ptr, 1 << 20, None) == E_ARG
    assert es(h, a.ptr, one, 0, b.ptr, 1 << 20, out3) == E_ARG and es(h, a.ptr, zero, 3, b.ptr, 1 << 20, out3) == E_ARG
    assert es(h, a.ptr, big, 3, b.ptr, 1 << 20, out3) == E_RANGE                              # the lengths alone decide
    assert es(h, a.ptr, arr(600, 400), 2, a.ptr + 992, 1 << 20, out3) == E_ARG                # overlap
    assert ds(h, None, sb, one, 1, c.ptr) == E_ARG and ds(h, b.ptr, None, one, 1, c.ptr) == E_ARG and ds(h, b.ptr, sb, None, 1, c.ptr) == E_ARG
    assert ds(h, b.ptr, sb, one, 1, None) == E_ARG and ds(h, b.ptr, sb, one, 0, c.ptr) == E_ARG and ds(h, b.ptr, sb, zero, 3, c.ptr) == E_ARG
    assert ds(h, b.ptr, sb, big, 3, c.ptr) == E_RANGE
    assert ds(h, b.ptr, sb, arr(5, 5, 5), 3, b.ptr + 1600) == E_ARG                           # overlap
    assert not host.any() and list(out3) == [0, 0, 0]
    assert ctx.ec_decode_device(b, size, c, 1000) == 1000                                     # the context still works


def test_timings(ctx, bufs, plan):
    T, K = plan
    a, b, c = bufs
    rng = np.random.default_rng(12)
    n = K * T + 3 * T + 1
    a.upload(_ranks(rng, n))
    ls = [T + 1, K * T + 2 * T]
    ctx.set_timing(2)
    try:
        got = {}
        calls = [(lambda: got.update(size=ctx.ec_encode_device(a, n, b, 4 * n)), 5),
                 (lambda: ctx.ec_decode_device(b, got["size"], c, n), 3),
                 (lambda: got.update(sizes=ctx.ec_encode_segments_device(a, ls, b, 4 * n)), 7),
                 (lambda: ctx.ec_decode_segments_device(b, got["sizes"], ls, c), 4)]
        for call, launches in calls:
            call()
            t = ctx.timings()
            k = t.as_dict()["kernels"]
            assert t.n == n and t.total_ms > 0 and set(k) == {"other"}
            spans = ctx.debug_last_spans()
            assert k["other"]["launches"] == len(spans) == launches and all(ms >= 0 for ms in spans)
            assert abs(sum(spans) - k["other"]["ms"]) < 1e-3
    finally:
        ctx.set_timing(0)
    ctx.ec_encode_device(a, n, b, 4 * n)
    assert ctx.debug_last_spans() == []                          # timing off: no launch is timed
    k = ctx.timings().as_dict()["kernels"]
    assert set(k) == {"other"} and k["other"]["launches"] == 5
