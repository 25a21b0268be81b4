"""GPU suite of version 2 of the member frame (include/bwts_members.h): the device's and the host form's frame byte for byte against the
CPU model (tests/pack_members_v2_model.py) on a member set with mixed widths and filters; unpack, range reads across a filtered /
unfiltered seam, member reads and bwts_frame_members_f against the model; no filter gives the version-1 bytes; the malformed
version-2 frames with the model's codes; a flipped filter bit is a checksum error; the memory kept; the capacity contract."""
import ctypes

import numpy as np
import pytest

import delta_model as D
import members_v2_cases as C2
import pack_members_model as MM
import pack_members_v2_model as M2
from test_pack_gpu import _first_diff, _u8

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
N = sum(C2.LENGTHS)
MARK = 0xA5


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame, as large as the bound of the member set; c: output"""
    a, c = ctx.alloc(N + 256), ctx.alloc(2 * N + 256)
    b = ctx.alloc(pkg.pack_members_bound(C2.LENGTHS) + 256)
    yield a, b, c
    for d in (a, b, c):
        d.free()


@pytest.fixture(scope="module")
def reference():
    """The member set, its concatenation and the model's frame: made once, shared, left unchanged."""
    members, widths, filters = C2.member_set()
    return members, widths, filters, _u8(b"".join(members)), _u8(C2.member_frame())


def test_pack_is_the_models_frame(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, filters, x, want = reference
    a.upload(x)
    cap = pkg.pack_members_bound(C2.LENGTHS)
    size = ctx.pack_members_device(a, C2.LENGTHS, widths, b, cap, filters=filters)
    y = b.download(size)
    assert size == want.size and np.array_equal(y, want), "pack: %s" % _first_diff(y, want)
    assert ctx.timings().n == N and ctx.timings().total_ms > 0
    f = ctx.pack_members(members, widths, filters)
    assert np.array_equal(f, want), "host pack: %s" % _first_diff(f, want)
    assert pkg.frame_members(f) == (C2.LENGTHS, widths) and pkg.frame_member_filters(f) == filters and pkg.unpack_size(f) == (N, f.size)
    # one member goes through the single-input stages: filtered at width 8, and at width 1 (no split at all)
    for k in (5, 7):
        one = ctx.pack_members([members[k]], [widths[k]], [1])
        assert one.tobytes() == M2.pack([members[k]], [widths[k]], [1]), k
        assert ctx.unpack(one).tobytes() == members[k]
    # numpy arrays are taken as their bytes; the filter is the caller's word
    one = ctx.pack_members([np.frombuffer(members[8][:16384], dtype="<i4")], [4], [pkg.FILTER_DELTA])
    assert one.tobytes() == M2.pack([members[8][:16384]], [4], [1])


def test_no_filter_is_the_version_1_frame(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, filters, x, want = reference
    a.upload(x)
    plain = MM.pack(members, widths)
    cap = pkg.pack_members_bound(C2.LENGTHS)
    for fs in (None, [0] * len(members)):
        size = ctx.pack_members_device(a, C2.LENGTHS, widths, b, cap, filters=fs)
        assert size == len(plain) and b.download(size).tobytes() == plain
        assert ctx.pack_members(members, widths, fs).tobytes() == plain
    assert pkg.frame_member_filters(plain) == [0] * len(members)
    assert ctx.pack_members(members, None, [0] * len(members)).tobytes() == MM.pack(members, None)


def test_unpack_and_members_against_the_model(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, filters, x, want = reference
    b.upload(want)
    c.upload(np.full(N + 64, MARK, dtype=np.uint8))
    assert ctx.unpack_device(b, want.size, c, N + 5) == N
    back = c.download(N + 64)
    assert np.array_equal(back[:N], x), "unpack: %s" % _first_diff(back[:N], x)
    assert (back[N:] == MARK).all() and ctx.timings().n == N
    assert ctx.unpack(want).tobytes() == x.tobytes() == M2.unpack(want.tobytes())
    perm = [7, 0, 5, 9, 5, 2]
    assert ctx.unpack_members(want, perm) == M2.unpack_members(want.tobytes(), perm) == [members[k] for k in perm]
    assert ctx.unpack_members(want) == members
    total = sum(C2.LENGTHS[k] for k in perm)
    c.upload(np.full(total + 64, MARK, dtype=np.uint8))
    assert ctx.unpack_members_device(b, want.size, perm, c, total) == total
    got = c.download(total + 64)
    assert got[:total].tobytes() == b"".join(members[k] for k in perm) and (got[total:] == MARK).all()
    r = ctx.debug_unpack_ranges_report()
    assert r["blocks"] == 5 and r["covered_bytes"] == sum(C2.LENGTHS[k] for k in set(perm)) and "delta" in r["stages"] and "join" in r["stages"]
    # one filtered member of width 1: the delta decode, and no join; one unfiltered member: neither
    for k, stages in ((7, {"delta"}), (6, set()), (5, {"delta", "join"}), (4, {"join"})):
        assert ctx.unpack_members_device(b, want.size, [k], c, C2.LENGTHS[k]) == C2.LENGTHS[k] and c.download(C2.LENGTHS[k]).tobytes() == members[k]
        r = ctx.debug_unpack_ranges_report()
        assert r["single"] and set(r["stages"]) & {"delta", "join"} == stages, (k, r)


def test_ranges_across_the_seams(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, filters, x, want = reference
    b.upload(want)
    f = want.tobytes()
    for name, rs in C2.range_sets():
        total = sum(nb for _, nb in rs)
        c.upload(np.full(total + 64, MARK, dtype=np.uint8))
        assert ctx.unpack_ranges_device(b, want.size, rs, c, total) == total, name
        got = c.download(total + 64)
        assert got[:total].tobytes() == b"".join(M2.unpack_ranges(f, rs)) == b"".join(x[o:o + nb].tobytes() for o, nb in rs), name
        assert (got[total:] == MARK).all(), name
        assert [g.tobytes() for g in ctx.unpack_ranges(want, rs)] == M2.unpack_ranges(f, rs), name
    # a range inside an unfiltered member alone runs no delta stage
    off = sum(C2.LENGTHS[:6])
    assert ctx.unpack_ranges_device(b, want.size, [(off + 5, 100)], c, 100) == 100 and c.download(100).tobytes() == members[6][5:105]
    assert "delta" not in ctx.debug_unpack_ranges_report()["stages"]


def test_malformed_version_2_frames(pkg, ctx, bufs):
    a, b, c = bufs
    x, f, cases = C2.malformed_cases()
    got = ctypes.c_uint64(0)
    n = len(x)
    every = np.arange(4, dtype=np.uint64)
    whole = np.array([(0, n)], dtype=np.uint64)
    for name, bad, code in [("valid", f, 0)] + cases:
        try:
            M2.unpack(bad)
            model = 0
        except MM.PackError as e:
            model = e.code
        assert model == code, name
        b.upload(_u8(bad))
        c.upload(np.full(n + 64, MARK, dtype=np.uint8))
        rc = pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(bad), c.ptr, n + 4096, ctypes.byref(got))
        assert rc == code, "%s: %d, the model says %d" % (name, rc, code)
        if code == 0:
            assert c.download(n).tobytes() == x
        c.upload(np.full(n + 64, MARK, dtype=np.uint8))
        rc = pkg.lib().bwts_unpack_ranges_device(ctx._h, b.ptr, len(bad), whole.ctypes.data, 1, c.ptr, n, ctypes.byref(got))
        assert rc == code, "%s: ranges %d, the model says %d" % (name, rc, code)
        if code:
            assert (c.download(n + 64) == MARK).all(), "%s: the range read failed, but something was written" % name
        rc = pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, len(bad), every.ctypes.data, 4, c.ptr, n, ctypes.byref(got))
        assert rc == code, "%s: members %d, the model says %d" % (name, rc, code)
        if code:
            assert (c.download(n + 64) == MARK).all(), "%s: the member read failed, but something was written" % name
            out = np.full(n + 16, 0x5A, dtype=np.uint8)
            with pytest.raises(pkg.BwtsError) as e:
                ctx.unpack(bad, out=out)
            assert e.value.code == code and (out == 0x5A).all(), name
    # a flipped filter bit leaves the frame canonical: it decodes in bounds and fails its checksum; members it does not touch are read
    by_name = {name: bad for name, bad, _ in cases}
    for name in ("a filter set on an unfiltered member", "a filter cleared, another one left"):
        b.upload(_u8(by_name[name]))
        assert pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(f), c.ptr, n, ctypes.byref(got)) == E_CHECKSUM
        idx = np.array([3, 2], dtype=np.uint64)
        assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, len(f), idx.ctypes.data, 2, c.ptr, 109, ctypes.byref(got)) == 0
        assert c.download(109).tobytes() == x[-9:] + x[8192:8292]
    # the context still works
    b.upload(_u8(f))
    assert ctx.unpack_device(b, len(f), c, n) == n and c.download(n).tobytes() == x


def test_memory_kept(pkg, reference):
    """device_bytes after a version-2 pack and after the unpack of its frame are those of the version-1 frame of the same lengths: two
    n-byte blocks for a pack, one for an unpack, and no more.  (What the transform takes depends on the bytes it sees, so version 1
    packs the filtered bytes here.)"""
    members, widths, filters, x, want = reference
    filtered = _u8(D.encode_segments(x, C2.LENGTHS, widths, filters).tobytes())
    kept = []
    for data, fs in ((filtered, None), (x, filters)):
        with pkg.Context(0) as c:
            a, s, back = c.alloc(N), c.alloc(pkg.pack_members_bound(C2.LENGTHS)), c.alloc(N)
            a.upload(data)
            size = c.pack_members_device(a, C2.LENGTHS, widths, s, s.nbytes, filters=fs)
            packed = c.timings().device_bytes
            c.release_memory()
            assert c.unpack_device(s, size, back, N) == N and np.array_equal(back.download(N), data)
            kept.append((packed, c.timings().device_bytes))
    assert kept[0] == kept[1], kept


def test_capacity_and_arguments(pkg, ctx, bufs, reference):
    """Exact capacity packs; one byte, or 16, short of the frame is BWTS_E_SPACE with nothing written at all."""
    a, b, c = bufs
    members, widths, filters, x, want = reference
    a.upload(x)
    size = want.size
    ls, ws, fs = np.array(C2.LENGTHS, dtype=np.uint64), np.array(widths, dtype=np.uint32), np.array(filters, dtype=np.uint32)
    mark = np.full(size + 64, MARK, dtype=np.uint8)
    b.upload(mark)
    assert ctx.pack_members_device(a, C2.LENGTHS, widths, b, size, filters=filters) == size
    assert np.array_equal(b.download(size + 64), np.concatenate((want, mark[size:])))
    got = ctypes.c_uint64(0)
    L, h = pkg.lib(), ctx._h
    for short in (1, 16, size - 32 - 32 * len(C2.LENGTHS)):
        b.upload(mark)
        rc = L.bwts_pack_members_f_device(h, a.ptr, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ls.size, b.ptr, size - short, ctypes.byref(got))
        assert rc == E_SPACE, (short, rc)
        assert np.array_equal(b.download(size + 64), mark), "BWTS_E_SPACE, but something was written"
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members(members, widths, filters, out_cap=size - 1)
    assert e.value.code == E_SPACE
    # a filter that is neither, with the bad widths; a filter list of another length
    bad = fs.copy()
    bad[3] = 2
    assert L.bwts_pack_members_f_device(h, a.ptr, ls.ctypes.data, ws.ctypes.data, bad.ctypes.data, ls.size, b.ptr, size, ctypes.byref(got)) == E_ARG
    assert L.bwts_pack_members_f_device(h, a.ptr, ls.ctypes.data, None, fs.ctypes.data, ls.size, b.ptr + 8, size, ctypes.byref(got)) == E_ARG
    assert L.bwts_pack_members_f_device(h, a.ptr, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, 0, b.ptr, size, ctypes.byref(got)) == E_ARG
    hp = np.zeros(64, dtype=np.uint8).ctypes.data
    assert L.bwts_pack_members_f(h, hp, ls.ctypes.data, ws.ctypes.data, bad.ctypes.data, ls.size, hp, 64, ctypes.byref(got)) == E_ARG
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members([b"abc", b"de"], [1, 1], [1])
    assert e.value.code == E_ARG
    # widths None with filters: every member filtered at width 1
    f1 = ctx.pack_members(members[:4], None, [1, 1, 1, 1])
    assert f1.tobytes() == M2.pack(members[:4], None, [1, 1, 1, 1]) and ctx.unpack(f1).tobytes() == b"".join(members[:4])
