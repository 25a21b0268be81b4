"""GPU suite of the checksum kernel (include/bwts_pack.h, csrc/crc.hip): bwts_crc32_device and its segment form against zlib.crc32 at
sizes taken from the engine's own plan (tile T, fold group G): the 16-byte piece, the tile ends, the group boundary and past two
groups; on uniform bytes, all zeros (the classic catch for a wrong length in the combine) and all 0xFF, from an aligned and an
unaligned start; the error contract; one input beyond 2^32 bytes whose value the model's combine predicts; and one segment table
through all three stages that share the segment cut and its table kernel (checksum, move-to-front, coder)."""
import ctypes
import zlib

import numpy as np
import pytest

import big_cases as B
import ec_model as E
import mtf_model as M
import pack_model as P

pytestmark = pytest.mark.gpu

E_ARG, E_NOMEM, E_RANGE = -1, -3, -5


@pytest.fixture(scope="module")
def plan(pkg):
    p = pkg.debug_crc_plan(1)
    return p["T"], p["G"]


def _sizes(plan):
    T, G = plan
    return [1, 2, 15, 16, 17, T - 1, T, T + 1, G * T - 1, G * T, G * T + 1, 2 * G * T + T + 7]


@pytest.fixture(scope="module")
def room(ctx, plan):
    T, G = plan
    d = ctx.alloc(2 * G * T + T + 7 + 64)
    yield d
    d.free()


@pytest.fixture(scope="module")
def references(plan):
    """content -> (the bytes of the largest size + 3, {(offset, n): zlib's value}): computed once, shared, left unchanged"""
    top = max(_sizes(plan)) + 3
    out = {}
    for name, x in (("uniform", np.random.default_rng(77).integers(0, 256, top, dtype=np.uint8)), ("zeros", np.zeros(top, dtype=np.uint8)),
                    ("ones", np.full(top, 0xFF, dtype=np.uint8))):
        x.setflags(write=False)
        out[name] = (x, {(off, n): zlib.crc32(x[off:off + n]) for n in _sizes(plan) for off in (0, 3)})
    return out


@pytest.mark.parametrize("name", ["uniform", "zeros", "ones"])
def test_every_size_against_zlib(ctx, plan, room, references, name):
    x, want = references[name]
    room.upload(x)
    for n in _sizes(plan):
        for off in (0, 3):
            got = ctx.crc32_device(room.ptr + off, n)
            assert got == want[(off, n)], "%s n=%d offset %d: %08x, zlib %08x" % (name, n, off, got, want[(off, n)])
    t = ctx.timings()
    assert t.n == _sizes(plan)[-1] and t.total_ms > 0


def test_every_alignment_of_a_short_input(ctx, room, references):
    x, _ = references["uniform"]
    room.upload(x[:4096])
    for off in range(17):
        for n in (1, 3, 4, 5, 16, 31, 33, 1024 + 5):
            assert ctx.crc32_device(room.ptr + off, n) == zlib.crc32(x[off:off + n]), (off, n)


def _segments_checked(ctx, room, x, lengths):
    room.upload(x)
    got = ctx.crc32_segments_device(room, lengths)
    at = 0
    for s, ln in enumerate(lengths):
        assert int(got[s]) == zlib.crc32(x[at:at + ln]), "segment %d of %d bytes at %d" % (s, ln, at)
        at += ln


def test_segments(ctx, plan, room, references):
    T, G = plan
    x, _ = references["uniform"]
    lengths = [1, 17, T, T + 1, 5, G * T + 3, 1]
    _segments_checked(ctx, room, x[:sum(lengths)], lengths)
    _segments_checked(ctx, room, np.zeros(sum(lengths), dtype=np.uint8), lengths)
    _segments_checked(ctx, room, x[:T + 1], [T + 1])                       # one segment: the table of one entry
    many = (1 + np.random.default_rng(5).integers(0, 300, 4096)).tolist()
    assert min(many) == 1 and max(many) == 300
    _segments_checked(ctx, room, x[:sum(many)], many)
    # the single call after a segmented one, and the other way round, on one context
    assert ctx.crc32_device(room, T + 5) == zlib.crc32(x[:T + 5])


WAVE_GRID_CAP = 2048        # workgroups of four waves the stages' shared table launch uses at most (csrc/device_utils.h, wave_grid)


def test_one_table_through_every_stage(pkg, ctx):
    """One segment table through the checksum, move-to-front and the coder on one context: the three stages cut it with one function
    (csrc/stage_cut.h) and write their per-unit tables with one kernel.  More segments than four times the launch's workgroup cap,
    and not a multiple of four, so the kernel's stride over segments runs and its last workgroup is not full; almost all of 1 to 17
    bytes; one of exactly 64 of the largest unit (the coder's block) and one, behind the stride, of 65, so the lanes' loop over a
    segment's units wraps for every stage."""
    mtf_T, crc_T, ec = pkg.debug_mtf_plan(1)["T"], pkg.debug_crc_plan(1)["T"], pkg.debug_ec_plan(1)
    unit = max(mtf_T, crc_T, ec["T"] * ec["K"])
    count = 4 * WAVE_GRID_CAP + 7
    assert unit == ec["T"] * ec["K"] == E.T * E.K and count % 4 != 0 and count > 4 * WAVE_GRID_CAP
    rng = np.random.default_rng(2024)
    lengths = 1 + rng.integers(0, 17, count)
    long64, long65 = 77, 4 * WAVE_GRID_CAP + 3
    lengths[long64], lengths[long65] = 64 * unit, 64 * unit + 1
    short = [s for s in range(count) if s not in (long64, long65)]
    assert min(lengths) == 1 and max(lengths[short]) == 17
    n = int(lengths.sum())
    offs = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    x = (rng.integers(0, 256, n, dtype=np.uint8) & rng.integers(0, 256, n, dtype=np.uint8))       # skewed: the ranks get a table worth coding
    cap = pkg.ec_bound_segments(lengths)
    a, b, c, coded = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(cap)
    try:
        a.upload(x)
        crcs = ctx.crc32_segments_device(a, lengths)
        bad = [s for s in range(count) if int(crcs[s]) != zlib.crc32(x[offs[s]:offs[s + 1]])]
        assert not bad, "checksum of segments %s ..." % bad[:8]
        # move-to-front: the model on every short segment, the round trip on all
        ctx.mtf_forward_segments_device(a, lengths, b)
        y = b.download(n)
        bad = [s for s in short if y[offs[s]:offs[s + 1]].tobytes() != M.forward(x[offs[s]:offs[s + 1]].tobytes())]
        assert not bad, "ranks of segments %s ..." % bad[:8]
        ctx.mtf_inverse_segments_device(b, lengths, c)
        assert np.array_equal(c.download(n), x)
        # the coder: the model's stream, and its size, on a handful of short segments; the round trip on all
        sizes = ctx.ec_encode_segments_device(b, lengths, coded, cap)
        soffs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        assert int(soffs[-1]) <= cap
        streams = coded.download(int(soffs[-1]))
        for s in (0, 1, long64 - 1, long64 + 1, 4 * WAVE_GRID_CAP - 1, 4 * WAVE_GRID_CAP, long65 - 1, long65 + 1, count - 1):
            want = E.encode(y[offs[s]:offs[s + 1]])
            assert int(sizes[s]) == len(want) and streams[soffs[s]:soffs[s + 1]].tobytes() == want, s
        ctx.ec_decode_segments_device(coded, sizes, lengths, c)
        assert np.array_equal(c.download(n), y)
    finally:
        for d in (a, b, c, coded):
            d.free()


def test_error_contract(pkg, ctx, room):
    L = pkg.lib()
    got = ctypes.c_uint32(0)
    arr = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    assert L.bwts_crc32_device(None, room.ptr, 5, ctypes.byref(got)) == E_ARG
    assert L.bwts_crc32_device(ctx._h, None, 5, ctypes.byref(got)) == E_ARG
    assert L.bwts_crc32_device(ctx._h, room.ptr, 5, None) == E_ARG
    assert L.bwts_crc32_device(ctx._h, room.ptr, 0, ctypes.byref(got)) == E_ARG
    assert L.bwts_crc32_device(ctx._h, room.ptr, (1 << 36) + 1, ctypes.byref(got)) == E_RANGE       # before the data is touched
    out = (ctypes.c_uint32 * 4)()
    assert L.bwts_crc32_segments_device(ctx._h, None, arr(5), 1, out) == E_ARG
    assert L.bwts_crc32_segments_device(ctx._h, room.ptr, None, 1, out) == E_ARG
    assert L.bwts_crc32_segments_device(ctx._h, room.ptr, arr(5), 0, out) == E_ARG
    assert L.bwts_crc32_segments_device(ctx._h, room.ptr, arr(5), 1, None) == E_ARG
    assert L.bwts_crc32_segments_device(ctx._h, room.ptr, arr(5, 0, 5), 3, out) == E_ARG
    assert L.bwts_crc32_segments_device(ctx._h, room.ptr, arr(1 << 31, 1 << 31, 1), 3, out) == E_RANGE


def _crc_of_copies(crc_one, length, q):
    """crc32 of q copies of a string from the crc32 of one, by doubling."""
    acc, acc_len = 0, 0                      # of the empty string
    piece, piece_len = crc_one, length
    while q:
        if q & 1:
            acc, acc_len = P.crc32_combine(acc, piece, piece_len), acc_len + piece_len
        piece, piece_len = P.crc32_combine(piece, piece, piece_len), 2 * piece_len
        q >>= 1
    return acc


def test_crc_of_copies_helper():
    s = b"seven blocks"
    assert _crc_of_copies(zlib.crc32(s), len(s), 1) == zlib.crc32(s) and _crc_of_copies(zlib.crc32(s), len(s), 37) == zlib.crc32(s * 37)


def test_beyond_2p32(pkg, ctx):
    """N_SINGLE bytes of the 1.75 MiB period, which does not divide 2^32: a read 2^32 short fetches other bytes."""
    per, n = B.period()[:B.P7], B.N_SINGLE
    want = P.crc32_combine(_crc_of_copies(zlib.crc32(per), B.P7, n // B.P7), zlib.crc32(per[:n % B.P7]), n % B.P7)
    try:
        d = ctx.alloc(n)
    except pkg.BwtsError as e:
        if e.code == E_NOMEM:
            pytest.skip("the device cannot hold %d bytes" % n)
        raise
    try:
        B.upload_periodic(pkg, ctx, d.ptr, per, n)
        assert ctx.crc32_device(d, n) == want
        assert ctx.crc32_device(d.ptr + 1, n - 1) != want
    finally:
        d.free()
