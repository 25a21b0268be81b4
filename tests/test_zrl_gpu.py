"""GPU suite of the zero-run stage (include/bwts_zrl.h): every output byte for byte against the CPU model (tests/zrl_model.py), the
device's and the model's bytes decoded on the device back to the input, built inputs for every tile-boundary case, the segment
forms, malformed inputs (each refused by the model first) with guard bytes around the output, the capacity contract, the error table
and the memory a call keeps.  The tile size comes from the engine's own plan."""
import ctypes

import numpy as np
import pytest

import zrl_model as Z
from test_zrl_model import dense_wide, ranks, run_boundaries, with_coded_size

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE = -1, -5, -8, -9
GUARD = 256


@pytest.fixture(scope="module")
def T(pkg):
    return pkg.debug_zrl_plan(1)["T"]


@pytest.fixture(scope="module")
def bufs(ctx):
    """a, c: the ranks' side; b: the coded side; all as large as the largest input (the runs of every digit count: 3 * 2^22 bytes and
    a few), with room for guard bytes"""
    cap = 13 << 20
    a, b, c = ctx.alloc(cap), ctx.alloc(cap), ctx.alloc(cap)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def _u8(x):
    return x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


def _first_diff(y, want):
    if y.size != want.size:
        return "sizes %d and %d" % (y.size, want.size)
    return "first difference at %d of %d" % (int(np.flatnonzero(y != want)[0]), y.size)


def _checked(ctx, bufs, x, off=0):
    """One input: device output == model output, device decode of both == x; off moves all three buffers off their alignment."""
    x = _u8(x)
    n = x.size
    a, b, c = (d.ptr + off for d in bufs)
    A, B, C = bufs
    want = _u8(Z.encode(x))
    A.upload(np.concatenate((np.zeros(off, dtype=np.uint8), x)))
    B.upload(np.full(off + n + 64, 0xA5, dtype=np.uint8))
    size = ctx.zrl_encode_device(a, n, b, n)
    assert size == want.size, (n, size, want.size)
    y = B.download(off + n + 64)
    assert np.array_equal(y[off:off + size], want), "encode n=%d: %s" % (n, _first_diff(y[off:off + size], want))
    assert (y[:off] == 0xA5).all() and (y[off + size:] == 0xA5).all(), "encode n=%d wrote outside its output" % n
    C.upload(np.full(off + n + 64, 0xEE, dtype=np.uint8))
    ctx.zrl_decode_device(b, size, c, n)
    back = C.download(off + n + 64)
    assert np.array_equal(back[off:off + n], x), "decode n=%d: %s" % (n, _first_diff(back[off:off + n], x))
    assert (back[:off] == 0xEE).all() and (back[off + n:] == 0xEE).all(), "decode n=%d wrote outside its output" % n
    return want


def _sizes(T):
    return [1, 2, 3, T - 1, T, T + 1, 4 * T + 1, (1 << 20) + 1]


@pytest.mark.parametrize("kind", ["zipf", "text", "uniform256", "repeat", "ab"])
def test_ranks_of_every_size(ctx, bufs, T, kind):
    for n in _sizes(T):
        want = _checked(ctx, bufs, ranks(kind, n))
        if kind == "uniform256" and n > 64:
            assert want.size == n                       # stored


def test_all_zeros_of_every_size(ctx, bufs, T):
    for n in _sizes(T):
        want = _checked(ctx, bufs, np.zeros(n, dtype=np.uint8))
        assert want.size == min(n, (n + 1).bit_length() - 1)


def test_one_run_over_512_tiles(ctx, bufs, T):
    """One rank, then 8 MiB + 2 zeros: a run over all tiles of the encode, and in the decode one digit that stands for 2^22 zeros."""
    n = (8 << 20) + 3
    x = np.zeros(n, dtype=np.uint8)
    x[0] = 113
    want = _checked(ctx, bufs, x)
    assert want.size == 1 + 23 and n // T >= 512


def test_built_tile_boundaries(ctx, bufs, T):
    built = {}
    x = np.full(4 * T, 3, dtype=np.uint8)
    x[T - 1:2 * T + T + 1] = 0                   # from a tile's last byte, over one whole tile of zeros, to the first byte of the next
    built["run over a whole tile"] = x
    x = np.full(3 * T, 3, dtype=np.uint8)
    x[T - 100:T] = 0                             # a run that ends with its tile; a rank opens the next
    built["run ends with its tile"] = x
    x = np.zeros(3 * T + 9, dtype=np.uint8)
    x[T] = 9                                     # zeros up to a tile's end, the rank first in the next, zeros to the end
    built["rank opens a tile between runs"] = x
    x = np.zeros(3 * T + 64, dtype=np.uint8)
    x[63::64] = 5                                # every thread's chunk ends with a rank
    x[64 * 7:64 * 9] = 0                         # ... but for a run over two whole chunks
    built["chunk boundaries"] = x
    built["every digit count"] = run_boundaries()
    built["dense 253 254 255"] = dense_wide(4 * T + 3)
    built["255 last"] = dense_wide(2 * T, last=255)
    built["254 last"] = dense_wide(2 * T + 1, last=254)
    for name, x in built.items():
        want = _checked(ctx, bufs, x)
        assert want.size < x.size, name
    # an escape pair across a coded tile's boundary: ranks of one byte each up to coded byte T - 1, which is the 255 of a pair
    for lead in (T - 1, T - 2, T):
        x = np.concatenate((np.full(lead, 9, dtype=np.uint8), [255, 254, 255], np.zeros(40 * T, dtype=np.uint8), [255]))
        z = _checked(ctx, bufs, x)
        assert z.size < x.size and z[lead] == 255 and z[lead + 1] == 1
    # a digit sequence across a coded tile's boundary, for the decoder's look-back: the digits of one long run start k bytes in front of it
    for k in (1, 5, 17, 19):
        x = np.concatenate((np.full(T - k, 9, dtype=np.uint8), np.zeros((1 << 19) + 5, dtype=np.uint8), [200], np.zeros(7, dtype=np.uint8)))
        z = _checked(ctx, bufs, x)
        assert (z[T - k:T + 19 - k] <= 1).all() and z[T + 19 - k] == 201
    # ... and a payload directly in front of a boundary digit: the digit's index is 0
    x = np.concatenate((np.full(T - 2, 9, dtype=np.uint8), [255], np.zeros((1 << 18) + 1, dtype=np.uint8)))
    z = _checked(ctx, bufs, x)
    assert z[T - 2] == 255 and z[T - 1] == 1 and z[T] <= 1


def test_coded_size_next_to_n(ctx, bufs, T):
    for n in (20, T + 1, 3 * T + 2):
        assert _checked(ctx, bufs, with_coded_size(n, -1)).size == n - 1
        for delta in (0, 1):
            x = with_coded_size(n, delta)
            assert np.array_equal(_checked(ctx, bufs, x), x)            # stored


def test_off_every_alignment(ctx, bufs, T):
    x = ranks("text", 4 * T + 1)
    u = ranks("uniform256", T + 5)
    for off in (1, 2, 3, 7, 8, 13, 15):
        _checked(ctx, bufs, x, off=off)
        _checked(ctx, bufs, u, off=off)


def _segments_checked(ctx, bufs, x, lengths, off=0):
    x = _u8(x)
    ls = np.asarray(lengths, dtype=np.uint64)
    n = int(ls.sum())
    assert n == x.size
    A, B, C = bufs
    a, b, c = (d.ptr + off for d in bufs)
    want = Z.encode_segments(x, ls.tolist())
    want_sizes = np.array([len(s) for s in want], dtype=np.uint64)
    total = int(want_sizes.sum())
    wcat = _u8(b"".join(want))
    A.upload(np.concatenate((np.zeros(off, dtype=np.uint8), x)))
    B.upload(np.full(off + n + 64, 0xA5, dtype=np.uint8))
    sizes = ctx.zrl_encode_segments_device(a, ls, b, n)
    assert np.array_equal(sizes, want_sizes)
    y = B.download(off + n + 64)
    assert np.array_equal(y[off:off + total], wcat), "segments: %s" % _first_diff(y[off:off + total], wcat)
    assert (y[:off] == 0xA5).all() and (y[off + total:] == 0xA5).all()
    C.upload(np.full(off + n + 64, 0xEE, dtype=np.uint8))
    ctx.zrl_decode_segments_device(b, sizes, ls, c)
    back = C.download(off + n + 64)
    assert np.array_equal(back[off:off + n], x), "segments decode: %s" % _first_diff(back[off:off + n], x)
    assert (back[:off] == 0xEE).all() and (back[off + n:] == 0xEE).all()
    # each segment byte for byte the single call's, both directions
    offs = np.concatenate(([0], np.cumsum(ls))).astype(np.int64)
    zoffs = np.concatenate(([0], np.cumsum(want_sizes))).astype(np.int64)
    for i in range(ls.size):
        o, zo, ln, sz = int(offs[i]), int(zoffs[i]), int(ls[i]), int(want_sizes[i])
        assert ctx.zrl_encode_device(a + o, ln, C, ln) == sz and np.array_equal(C.download(sz), wcat[zo:zo + sz]), i
        ctx.zrl_decode_device(b + zo, sz, C, ln)
        assert np.array_equal(C.download(ln), x[o:o + ln]), i
    # exact capacity (one byte less: test_segments)
    assert np.array_equal(ctx.zrl_encode_segments_device(a, ls, b, total), want_sizes)
    return sizes, total


def test_segments(pkg, ctx, bufs, T):
    L = pkg.lib()
    rng = np.random.default_rng(7)
    lengths = [1, 1, T, T + 1, 5, 3 * T - 1, 4096, 2]
    n = sum(lengths)
    sparse = np.where(rng.random(n) < 0.8, 0, rng.integers(1, 256, n)).astype(np.uint8)
    mixed = sparse.copy()
    o = np.concatenate(([0], np.cumsum(lengths)))
    mixed[o[3]:o[4]] = rng.integers(1, 256, lengths[3])          # one stored segment among coded ones, and the short ones
    mixed[o[6]:o[7]] = rng.integers(0, 256, lengths[6])
    ends = sparse.copy()
    for s in range(1, len(lengths)):                             # every segment ends in zeros and the next starts with zeros
        ends[max(o[s] - 3, o[s - 1]):min(o[s] + 3, o[s + 1])] = 0
    for x in (sparse, mixed, ends, np.zeros(n, dtype=np.uint8)):
        for off in (0, 5):
            sizes, total = _segments_checked(ctx, bufs, x, lengths, off=off)
    assert int(sizes[0]) == 1 and int(sizes[2]) == 14           # all zeros: T zeros are 14 digits
    # BWTS_E_SPACE one byte short: nothing is written
    a, b, c = bufs
    ls = np.asarray(lengths, dtype=np.uint64)
    out = np.zeros(ls.size, dtype=np.uint64)
    b.upload(np.full(n, 0xA5, dtype=np.uint8))
    assert L.bwts_zrl_encode_segments_device(ctx._h, a.ptr + 5, ls.ctypes.data, ls.size, b.ptr, total - 1, out.ctypes.data) == E_SPACE
    assert (b.download(n) == 0xA5).all() and not out.any()
    # the runs of neighbouring segments do not merge
    x = np.zeros(8, dtype=np.uint8)
    x[0], x[7] = 9, 8
    a.upload(x)
    sizes = ctx.zrl_encode_segments_device(a, [4, 4], b, 8)
    assert sizes.tolist() == [3, 3] and b.download(6).tolist() == [10, 0, 0, 0, 0, 9]
    # many short segments
    lengths = rng.integers(1, 200, 3000)
    n = int(lengths.sum())
    _segments_checked(ctx, bufs, np.where(rng.random(n) < 0.9, 0, rng.integers(1, 256, n)).astype(np.uint8), lengths)


def test_segments_wrong_lengths_are_a_format_error(pkg, ctx, bufs, T):
    rng = np.random.default_rng(9)
    lengths = [T - 1, 7, T + 1]
    n = sum(lengths)
    x = np.where(rng.random(n) < 0.8, 0, rng.integers(1, 256, n)).astype(np.uint8)
    a, b, c = bufs
    a.upload(x)
    sizes = ctx.zrl_encode_segments_device(a, lengths, b, n)
    z = b.download(int(sizes.sum())).tobytes()
    for wrong in ([T - 1, 8, T], [T, 7, T], [T - 2, 7, T + 2]):       # the sums agree, the segments do not
        assert Z.decode_segments(z, sizes.tolist(), wrong) is None
        with pytest.raises(pkg.BwtsError) as e:
            ctx.zrl_decode_segments_device(b, sizes, wrong, c)
        assert e.value.code == E_FORMAT, wrong
    ctx.zrl_decode_segments_device(b, sizes, lengths, c)
    assert np.array_equal(c.download(n), x)


def test_malformed_inputs(pkg, ctx, bufs):
    L = pkg.lib()
    a, b, c = bufs
    for name, z, n in Z.malformed_cases():
        assert Z.decode(z, n) is None, name                        # the model refuses it first
        if n > (8 << 20):
            continue                                               # (the 2^36 case of the CPU suite: no buffer is that long)
        b.upload(np.concatenate((_u8(z), np.zeros(64, dtype=np.uint8))))
        c.upload(np.full(n + 2 * GUARD, 0xEE, dtype=np.uint8))
        rc = L.bwts_zrl_decode_device(ctx._h, b.ptr, len(z), c.ptr + GUARD, n)
        assert rc == E_FORMAT, (name, rc)
        got = c.download(n + 2 * GUARD)
        assert (got[:GUARD] == 0xEE).all() and (got[GUARD + n:] == 0xEE).all(), name
        # ... and as one segment among good ones
        good = bytes([5, 0, 1, 3, 255, 1, 0, 0])
        if len(z) <= n:
            ils = np.array([len(good), len(z), len(good)], dtype=np.uint64)
            ls = np.array([11, n, 11], dtype=np.uint64)
            b.upload(_u8(good + z + good))
            c.upload(np.full(n + 22 + 2 * GUARD, 0xEE, dtype=np.uint8))
            rc = L.bwts_zrl_decode_segments_device(ctx._h, b.ptr, ils.ctypes.data, ls.ctypes.data, 3, c.ptr + GUARD)
            assert rc == E_FORMAT, (name, rc)
            got = c.download(n + 22 + 2 * GUARD)
            assert (got[:GUARD] == 0xEE).all() and (got[GUARD + n + 22:] == 0xEE).all(), name
    # the context still works
    _checked(ctx, bufs, bytes([4, 0, 0, 0, 0, 0, 2, 255, 0, 0, 0]))


def test_space_contract(pkg, ctx, bufs, T):
    L = pkg.lib()
    a, b, c = bufs
    got = ctypes.c_uint64(77)
    for x in (ranks("text", 4 * T + 1), ranks("uniform256", T + 5)):
        n = x.size
        size = len(Z.encode(x))
        a.upload(x)
        mark = np.full(n + 64, 0xA5, dtype=np.uint8)
        b.upload(mark)
        assert ctx.zrl_encode_device(a, n, b, size) == size                      # exact capacity
        assert (b.download(n + 64)[size:] == 0xA5).all()
        b.upload(mark)
        assert L.bwts_zrl_encode_device(ctx._h, a.ptr, n, b.ptr, size - 1, ctypes.byref(got)) == E_SPACE
        assert (b.download(n + 64) == 0xA5).all() and got.value == 77            # marks everywhere


def test_host_forms(pkg, ctx, T):
    L = pkg.lib()
    x = ranks("text", (1 << 20) + 1)
    z = ctx.zrl_encode(x)
    assert z.tobytes() == Z.encode(x)
    assert ctx.timings().n == x.size
    assert np.array_equal(ctx.zrl_decode(z, x.size), x)
    assert ctx.timings().n == x.size
    u = ranks("uniform256", T + 5)
    assert np.array_equal(ctx.zrl_encode(u), u) and np.array_equal(ctx.zrl_decode(u, u.size), u)
    got = ctypes.c_uint64(77)
    out = np.full(x.size, 0x3C, dtype=np.uint8)
    assert L.bwts_zrl_encode(ctx._h, x.ctypes.data, x.size, out.ctypes.data, z.size - 1, ctypes.byref(got)) == E_SPACE
    assert (out == 0x3C).all() and got.value == 77
    bad = z.copy()
    bad[bad.size // 2] = 255
    bad[bad.size // 2 + 1] = 7
    assert Z.decode(bad, x.size) is None
    assert L.bwts_zrl_decode(ctx._h, bad.ctypes.data, bad.size, out.ctypes.data, x.size) == E_FORMAT
    assert (out == 0x3C).all()


def test_errors(pkg, ctx, bufs):
    L = pkg.lib()
    a, b, c = bufs
    got = ctypes.c_uint64(0)
    g = ctypes.byref(got)
    h = ctx._h
    enc, dec = L.bwts_zrl_encode_device, L.bwts_zrl_decode_device
    a.upload(np.zeros(4096, dtype=np.uint8))
    assert ctx.zrl_encode_device(a, 1000, b, 1000) == 9
    assert enc(None, a.ptr, 1000, b.ptr, 1000, g) == E_ARG and enc(h, None, 1000, b.ptr, 1000, g) == E_ARG and enc(h, a.ptr, 1000, None, 1000, g) == E_ARG
    assert enc(h, a.ptr, 1000, b.ptr, 1000, None) == E_ARG and enc(h, a.ptr, 0, b.ptr, 1000, g) == E_ARG
    assert enc(h, a.ptr, 1000, a.ptr + 999, 1000, g) == E_ARG and enc(h, a.ptr, 1000, a.ptr - 10, 11, g) == E_ARG        # overlap
    assert enc(h, a.ptr, 1000, a.ptr + 992, (1 << 64) - 1, g) == E_ARG                                                  # ... no wrap
    assert enc(h, a.ptr, (1 << 36) + 1, b.ptr, 1 << 20, g) == E_RANGE
    assert dec(None, b.ptr, 9, c.ptr, 1000) == E_ARG and dec(h, None, 9, c.ptr, 1000) == E_ARG and dec(h, b.ptr, 9, None, 1000) == E_ARG
    assert dec(h, b.ptr, 0, c.ptr, 1000) == E_ARG and dec(h, b.ptr, 9, c.ptr, 0) == E_ARG
    assert dec(h, b.ptr, 9, b.ptr + 8, 1000) == E_ARG and dec(h, b.ptr, 9, b.ptr - 999, 1000) == E_ARG                  # overlap
    assert dec(h, b.ptr, 9, c.ptr, (1 << 36) + 1) == E_RANGE
    assert dec(h, b.ptr, 10, c.ptr, 9) == E_FORMAT
    host = np.zeros(4096, dtype=np.uint8)
    hp = host.ctypes.data
    assert L.bwts_zrl_encode(h, None, 16, hp, 4096, g) == E_ARG and L.bwts_zrl_encode(h, hp, 16, None, 4096, g) == E_ARG
    assert L.bwts_zrl_encode(h, hp, 0, hp, 4096, g) == E_ARG and L.bwts_zrl_encode(h, hp, 16, hp, 4096, None) == E_ARG
    assert L.bwts_zrl_encode(None, hp, 16, hp, 4096, g) == E_ARG and L.bwts_zrl_encode(h, hp, (1 << 36) + 1, hp, 4096, g) == E_RANGE
    assert L.bwts_zrl_decode(h, None, 16, hp, 4096) == E_ARG and L.bwts_zrl_decode(h, hp, 16, None, 4096) == E_ARG
    assert L.bwts_zrl_decode(h, hp, 0, hp, 4096) == E_ARG and L.bwts_zrl_decode(None, hp, 16, hp, 4096) == E_ARG
    assert L.bwts_zrl_decode(h, hp, 17, hp, 16) == E_FORMAT
    arr = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    one, zero, big, il = arr(5), arr(5, 0, 5), arr(1 << 31, 1 << 31, 1), arr(3, 3, 3)
    out3 = arr(0, 0, 0)
    es, ds = L.bwts_zrl_encode_segments_device, L.bwts_zrl_decode_segments_device
    assert es(h, None, one, 1, b.ptr, 1 << 20, out3) == E_ARG and es(h, a.ptr, one, 1, None, 1 << 20, out3) == E_ARG
    assert es(h, a.ptr, None, 1, b.ptr, 1 << 20, out3) == E_ARG and es(h, a.ptr, one, 1, b.ptr, 1 << 20, None) == E_ARG
    assert es(h, a.ptr, one, 0, b.ptr, 1 << 20, out3) == E_ARG and es(h, a.ptr, zero, 3, b.ptr, 1 << 20, out3) == E_ARG
    assert es(h, a.ptr, big, 3, b.ptr, 1 << 20, out3) == E_RANGE                              # the lengths alone decide
    assert es(h, a.ptr, arr(600, 400), 2, a.ptr + 992, 1 << 20, out3) == E_ARG                # overlap
    assert ds(h, None, il, one, 1, c.ptr) == E_ARG and ds(h, b.ptr, None, one, 1, c.ptr) == E_ARG and ds(h, b.ptr, il, None, 1, c.ptr) == E_ARG
    assert ds(h, b.ptr, il, one, 1, None) == E_ARG and ds(h, b.ptr, il, one, 0, c.ptr) == E_ARG and ds(h, b.ptr, il, zero, 3, c.ptr) == E_ARG
    assert ds(h, b.ptr, arr(3, 0, 3), arr(5, 5, 5), 3, c.ptr) == E_ARG
    assert ds(h, b.ptr, il, big, 3, c.ptr) == E_RANGE
    assert ds(h, b.ptr, arr(3, 6, 3), arr(5, 5, 5), 3, c.ptr) == E_FORMAT                     # a coded segment longer than its ranks
    assert ds(h, b.ptr, il, arr(5, 5, 5), 3, b.ptr + 8) == E_ARG                              # overlap
    assert not host.any() and list(out3) == [0, 0, 0]
    ctx.zrl_decode_device(b, 9, c, 1000)                                                      # the context still works
    assert not c.download(1000).any()


def test_timings_and_memory_behind_move_to_front(ctx, bufs, T):
    """n and total_ms are filled, the kernels are booked under "other"; a zero-run call behind a move-to-front call of the same
    bytes takes no device memory."""
    a, b, c = bufs
    n = (8 << 20) + 3
    x = np.zeros(n, dtype=np.uint8)
    x[::997] = 3
    a.upload(x)
    ctx.mtf_forward_device(a, n, c)
    kept = ctx.timings().device_bytes
    size = ctx.zrl_encode_device(c, n, b, n)
    t = ctx.timings()
    assert t.n == n and t.total_ms > 0 and set(t.as_dict()["kernels"]) == {"other"}
    assert t.device_bytes == kept
    ctx.zrl_decode_device(b, size, a, n)
    t = ctx.timings()
    assert t.n == n and t.total_ms > 0 and set(t.as_dict()["kernels"]) == {"other"}
    assert t.device_bytes == kept
    ctx.mtf_inverse_device(a, n, c)
    assert np.array_equal(c.download(n), x)
