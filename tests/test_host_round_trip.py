"""The one host round trip (csrc/staging.hip) behind every host-buffer entry point: each host form against its own _device form
(DeviceBuffer.upload, the device call, download), byte for byte, at sizes around the 8 MiB staging slot and the ring of four; the
timing fields; pinned caller blocks; the sink; the public staging knobs, which select the copy paths; a failed call leaves `out`
as it was.  At 4,099 bytes and below also against the oracle and the Python models.

A failed ec_decode (one payload bit flipped, E_FORMAT) and a failed unpack (a resealed frame with a wrong block CRC, E_CHECKSUM)
leaving `out` untouched are asserted by test_ec_gpu.py::test_host_forms and test_pack_gpu.py::test_host_forms; the pack case is here."""
import ctypes
import os

import numpy as np
import pytest

import ec_model as E
import mtf_model as M
import oracle_lib as O
import pack_model as P

pytestmark = pytest.mark.gpu

SLOT = 1 << 23
FIVE_CHUNKS = 4 * SLOT + 17                   # a slot is reused: the wait for its earlier copy runs
SIZES = [1, 4099, SLOT - 1, SLOT, SLOT + 1, FIVE_CHUNKS]          # 4099: the copy kernel has a 3-byte tail
CODED_SIZES = [4099, FIVE_CHUNKS]
SEGMENTS = [SLOT, 1, SLOT + 16]
E_SPACE = -9


@pytest.fixture(scope="module")
def data():
    x = np.ascontiguousarray(O.generate("zipf", FIVE_CHUNKS, 11), dtype=np.uint8)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    top = max(pkg.pack_bound(FIVE_CHUNKS, 1 << 22), pkg.pack_bound(FIVE_CHUNKS), pkg.ec_bound(FIVE_CHUNKS)) + 64
    a, b = ctx.alloc(top), ctx.alloc(top)
    yield a, b
    a.free()
    b.free()


def _timed(ctx, n):
    t = ctx.timings()
    assert t.n == n and t.h2d_ms > 0 and t.d2h_ms > 0, (n, t.n, t.h2d_ms, t.d2h_ms)


def _device(bufs, x, call):
    """x on the device, call(d_in, d_out) -> bytes made (None: as many as went in), and those back."""
    a, b = bufs
    a.upload(x)
    made = call(a, b)
    return b.download(x.size if made is None else made)


def _same(y, want, what):
    assert y.size == want.size and np.array_equal(y, want), "%s: %d and %d bytes%s" % (
        what, y.size, want.size, "" if y.size != want.size else ", first difference at %d" % int(np.flatnonzero(y != want)[0]))


@pytest.mark.parametrize("n", SIZES)
def test_transform_and_move_to_front(ctx, bufs, data, n):
    x = data[:n]
    pairs = (("forward", ctx.forward, ctx.forward_device, ctx.inverse, ctx.inverse_device, lambda v: O.forward(v)),
             ("mtf", ctx.mtf_forward, ctx.mtf_forward_device, ctx.mtf_inverse, ctx.mtf_inverse_device,
              lambda v: np.frombuffer(M.forward_fast(v.tobytes()), dtype=np.uint8)))
    for name, fwd, fwd_dev, inv, inv_dev, model in pairs:
        y = fwd(x)
        _timed(ctx, n)
        _same(y, _device(bufs, x, lambda a, b: fwd_dev(a, n, b)), "%s of %d bytes, host and device form" % (name, n))
        if n <= 4099:
            _same(y, np.asarray(model(x), dtype=np.uint8), "%s of %d bytes against the model" % (name, n))
        back = inv(y)
        _timed(ctx, n)
        _same(back, _device(bufs, y, lambda a, b: inv_dev(a, n, b)), "inverse %s of %d bytes, host and device form" % (name, n))
        _same(back, x, "inverse(%s(x)) of %d bytes" % (name, n))


@pytest.mark.parametrize("n", CODED_SIZES)
def test_coder_and_frame(pkg, ctx, bufs, data, n):
    x = data[:n]
    s = ctx.ec_encode(x)
    _timed(ctx, n)
    _same(s, _device(bufs, x, lambda a, b: ctx.ec_encode_device(a, n, b, pkg.ec_bound(n))), "stream of %d bytes" % n)
    if n <= 4099:
        assert s.tobytes() == E.encode(x.tobytes())
    back = ctx.ec_decode(s)
    _timed(ctx, n)
    _same(back, _device(bufs, s, lambda a, b: ctx.ec_decode_device(a, s.size, b, n)), "decoded stream of %d bytes" % n)
    _same(back, x, "ec_decode(ec_encode(x)) of %d bytes" % n)
    for block in (0, 1 << 22):                # one block; several (where n is above a block)
        f = ctx.pack(x, block)
        _timed(ctx, n)
        _same(f, _device(bufs, x, lambda a, b: ctx.pack_device(a, n, block, b, pkg.pack_bound(n, block))), "frame of %d bytes, block %d" % (n, block))
        if n <= 4099:
            assert f.tobytes() == P.pack(x.tobytes(), block)
        back = ctx.unpack(f)
        _timed(ctx, n)
        _same(back, _device(bufs, f, lambda a, b: ctx.unpack_device(a, f.size, b, n)), "unpacked frame of %d bytes, block %d" % (n, block))
        _same(back, x, "unpack(pack(x)) of %d bytes, block %d" % (n, block))
        # a frame that does not fit: refused by the device form, and nothing has reached out
        out = np.full(f.size, 0xEE, dtype=np.uint8)
        got = ctypes.c_uint64(77)
        assert pkg.lib().bwts_pack(ctx._h, x.ctypes.data, n, block, out.ctypes.data, f.size - 16, ctypes.byref(got)) == E_SPACE
        assert (out == 0xEE).all() and got.value == 77


def test_segments(ctx, bufs, data):
    n = sum(SEGMENTS)
    x = data[:n]
    y = ctx.forward_segments(x, SEGMENTS)
    _timed(ctx, n)
    _same(y, _device(bufs, x, lambda a, b: ctx.forward_segments_device(a, SEGMENTS, b)), "forward_segments, host and device form")
    back = ctx.inverse_segments(y, SEGMENTS)
    _timed(ctx, n)
    _same(back, _device(bufs, y, lambda a, b: ctx.inverse_segments_device(a, SEGMENTS, b)), "inverse_segments, host and device form")
    _same(back, x, "inverse_segments(forward_segments(x))")


def test_sink_and_pinned_blocks(ctx, data):
    x = data
    want = ctx.forward(x)
    _same(ctx.forward_sink(x), want, "the sink's pieces, put together")
    _timed(ctx, x.size)
    n = SLOT + 1
    want = ctx.forward(x[:n])
    a, pa = ctx.host_alloc(n)
    b, pb = ctx.host_alloc(n)
    try:
        a[:] = x[:n]
        b[:] = 0
        ctx.forward_into(a, b)
        _timed(ctx, n)
        _same(b, want, "forward, pinned in and out")
        out = np.zeros(n, dtype=np.uint8)
        ctx.forward_into(a, out)
        _timed(ctx, n)
        _same(out, want, "forward, pinned in, plain out")
    finally:
        del a, b
        ctx.host_free(pa)
        ctx.host_free(pb)


@pytest.mark.parametrize("knob,value", [("BWTS_D2H", "dma"), ("BWTS_D2H_SPLIT", "50"), ("BWTS_D2H_SPLIT", "0"), ("BWTS_H2D", "kernel"),
                                        ("BWTS_COPY_THREADS", "1")])
def test_staging_knobs(pkg, ctx, data, knob, value):
    """The knobs are read when the context is made; every copy path they select moves the same bytes as the default one."""
    want = ctx.forward(data)
    before = os.environ.get(knob)
    os.environ[knob] = value
    try:
        other = pkg.Context(0)
    finally:
        if before is None:
            del os.environ[knob]
        else:
            os.environ[knob] = before
    with other:
        y = other.forward(data)
        _timed(other, data.size)
        _same(y, want, "forward under %s=%s" % (knob, value))
        back = other.inverse(y)
        _timed(other, data.size)
        _same(back, data, "inverse under %s=%s" % (knob, value))
