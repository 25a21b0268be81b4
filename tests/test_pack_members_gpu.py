"""GPU suite of the member frame (include/bwts_members.h): the device's and the host form's frame byte for byte against the CPU model
(tests/pack_members_model.py) on the member set that meets every boundary; unpack, range reads and member reads against the model;
what a range read decodes; every malformed frame of the CPU suite with its code (each refused by the model with that code first),
and outputs left untouched where the header promises it; the capacity contract; one member; members that make a version-2 frame's
streams; the committed fixtures."""
import ctypes
import os

import numpy as np
import pytest

import members_cases as C
import pack_members_model as MM
import pack_v2_model as P2
from test_pack_gpu import _first_diff, _u8
from test_pack_model import fixture_input

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
N = sum(C.LENGTHS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARK = 0xA5


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame, as large as the bound of the member set; c: output"""
    a, c = ctx.alloc(N + 256), ctx.alloc(2 * N + 256)
    b = ctx.alloc(pkg.pack_members_bound(C.LENGTHS) + 256)
    yield a, b, c
    for d in (a, b, c):
        d.free()


@pytest.fixture(scope="module")
def reference():
    """The member set, its concatenation and the model's frame: made once, shared, left unchanged."""
    members, widths = C.member_set()
    return members, widths, _u8(b"".join(members)), _u8(C.member_frame())


def test_pack_is_the_models_frame(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, x, want = reference
    a.upload(x)
    cap = pkg.pack_members_bound(C.LENGTHS)
    assert cap == MM.bound(C.LENGTHS)
    size = ctx.pack_members_device(a, C.LENGTHS, widths, b, cap)
    y = b.download(size)
    assert size == want.size and np.array_equal(y, want), "pack: %s" % _first_diff(y, want)
    assert ctx.timings().n == N and ctx.timings().total_ms > 0
    # the host form, from arrays and from bytes
    f = ctx.pack_members(members, widths)
    assert np.array_equal(f, want), "host pack: %s" % _first_diff(f, want)
    assert pkg.frame_members(f) == (C.LENGTHS, widths) and pkg.unpack_size(f) == (N, f.size)
    # numpy arrays of another dtype are taken as their bytes, and the width is the caller's word
    k = C.LENGTHS.index(4096)
    one = ctx.pack_members([np.frombuffer(members[k], dtype="<f4")], [4])
    assert one.tobytes() == MM.pack([members[k]], [4])
    # widths None: no split anywhere
    plain = ctx.pack_members(members)
    assert plain.tobytes() == MM.pack(members, None)
    assert ctx.pack_members_device(a, C.LENGTHS, None, b, cap) == plain.size and np.array_equal(b.download(plain.size), plain)


def test_unpack_against_the_model(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, x, want = reference
    b.upload(want)
    c.upload(np.zeros(N, dtype=np.uint8))
    assert ctx.unpack_device(b, want.size, c, N + 5) == N
    back = c.download(N)
    assert np.array_equal(back, x), "unpack: %s" % _first_diff(back, x)
    assert ctx.timings().n == N
    assert ctx.unpack(want).tobytes() == x.tobytes()
    # members: a permutation with a repeat, a single index, all of them
    perm = [12, 0, 5, 7, 5, 3]
    assert ctx.unpack_members(want, perm) == MM.unpack_members(want.tobytes(), perm) == [members[k] for k in perm]
    assert ctx.unpack_members(want, [9]) == [members[9]]
    assert ctx.unpack_members(want) == members
    total = sum(C.LENGTHS[k] for k in perm)
    c.upload(np.full(total + 64, MARK, dtype=np.uint8))
    assert ctx.unpack_members_device(b, want.size, perm, c, total) == total
    got = c.download(total + 64)
    assert got[:total].tobytes() == b"".join(members[k] for k in perm) and (got[total:] == MARK).all()
    r = ctx.debug_unpack_ranges_report()
    assert r["blocks"] == 5 and r["covered_bytes"] == sum(C.LENGTHS[k] for k in set(perm)) and r["pieces"] == len(perm)      # a member is decoded once
    assert ctx.timings().n == r["covered_bytes"]
    assert ctx.unpack_members_device(b, want.size, [9], c, C.LENGTHS[9]) == C.LENGTHS[9] and c.download(C.LENGTHS[9]).tobytes() == members[9]
    r = ctx.debug_unpack_ranges_report()
    assert r["single"] and r["blocks"] == 1 and "join" in r["stages"] and C.WIDTHS[9] == 2


def test_ranges_against_the_model(pkg, ctx, bufs, reference):
    a, b, c = bufs
    members, widths, x, want = reference
    b.upload(want)
    f = want.tobytes()
    for name, rs in C.range_sets():
        p = MM.plan(f, rs)
        total = p["out_bytes"]
        c.upload(np.full(total + 64, MARK, dtype=np.uint8))
        assert ctx.unpack_ranges_device(b, want.size, rs, c, total) == total, name
        got = c.download(total + 64)
        assert got[:total].tobytes() == b"".join(x[o:o + nb].tobytes() for o, nb in rs), name
        assert (got[total:] == MARK).all(), name
        r = ctx.debug_unpack_ranges_report()
        # only the covered members are decoded
        assert (r["blocks"], r["runs"], r["covered_bytes"], r["stream_bytes"], r["pieces"]) == \
            (p["blocks"], len(p["runs"]), p["covered_bytes"], p["stream_bytes"], len(rs)), (name, r)
        assert r["gathered"] == (len(p["runs"]) > 1) and r["single"] == (p["blocks"] == 1), (name, r)
        assert ("join" in r["stages"]) == any(widths[k] != 1 for k in p["covered"]), (name, r)
        assert ctx.timings().n == p["covered_bytes"]
        assert pkg.debug_unpack_ranges_plan(f, rs)["runs"] == p["runs"], name
        assert [g.tobytes() for g in ctx.unpack_ranges(want, rs)] == MM.unpack_ranges(f, rs), name
    # a range in a member of width 1 alone: no join
    k = C.LENGTHS.index(4096)
    assert widths[k] == 1
    off = sum(C.LENGTHS[:k])
    assert ctx.unpack_ranges_device(b, want.size, [(off + 5, 100)], c, 100) == 100 and c.download(100).tobytes() == members[k][5:105]
    assert "join" not in ctx.debug_unpack_ranges_report()["stages"]
    # the ranges are judged behind the frame, before anything is written
    got = ctypes.c_uint64(0)
    c.upload(np.full(256, MARK, dtype=np.uint8))
    for rs, cap, code in (([(0, 0)], 256, E_ARG), ([(N, 1)], 256, E_RANGE), ([(N - 1, 2)], 256, E_RANGE), ([(0, 100), (5, 100)], 199, E_SPACE)):
        arr = np.array(rs, dtype=np.uint64)
        assert pkg.lib().bwts_unpack_ranges_device(ctx._h, b.ptr, want.size, arr.ctypes.data, len(rs), c.ptr, cap, ctypes.byref(got)) == code, rs
    for idx, cap, code in (([], 256, E_ARG), ([13], 256, E_RANGE), ([0, 1 << 40], 256, E_RANGE), ([1, 1], 3, E_SPACE)):
        arr = np.array(idx + [0], dtype=np.uint64)
        assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, want.size, arr.ctypes.data, len(idx), c.ptr, cap, ctypes.byref(got)) == code, idx
    assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, want.size, None, 1, c.ptr, 256, ctypes.byref(got)) == E_ARG
    assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr + 8, want.size, arr.ctypes.data, 1, c.ptr, 256, ctypes.byref(got)) == E_ARG      # d_in off 16 bytes
    assert (c.download(256) == MARK).all()


def test_malformed_frames(pkg, ctx, bufs):
    a, b, c = bufs
    x, f, cases = C.malformed_cases()
    got = ctypes.c_uint64(0)
    n = len(x)
    every = np.arange(4, dtype=np.uint64)
    whole = np.array([(0, n)], dtype=np.uint64)
    for name, bad, code in [("valid", f, 0)] + cases:
        try:
            MM.unpack(bad)
            model = 0
        except MM.PackError as e:
            model = e.code
        assert model == code, name                           # refused by the model, with this code, first
        b.upload(_u8(bad))
        rc = pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(bad), c.ptr, n + 4096, ctypes.byref(got))
        assert rc == code, "%s: %d, the model says %d" % (name, rc, code)
        # the range reader and the member reader give the same code, and write nothing when they fail
        c.upload(np.full(n + 64, MARK, dtype=np.uint8))
        rc = pkg.lib().bwts_unpack_ranges_device(ctx._h, b.ptr, len(bad), whole.ctypes.data, 1, c.ptr, n, ctypes.byref(got))
        assert rc == code, "%s: ranges %d, the model says %d" % (name, rc, code)
        if code:
            assert (c.download(n + 64) == MARK).all(), "%s: the range read failed, but something was written" % name
        c.upload(np.full(n + 64, MARK, dtype=np.uint8))
        rc = pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, len(bad), every.ctypes.data, 4, c.ptr, n, ctypes.byref(got))
        assert rc == code, "%s: members %d, the model says %d" % (name, rc, code)
        if code:
            assert (c.download(n + 64) == MARK).all(), "%s: the member read failed, but something was written" % name
        else:
            assert c.download(n).tobytes() == x
        # the host forms leave out as it was
        if code:
            out = np.full(n + 16, 0x5A, dtype=np.uint8)
            with pytest.raises(pkg.BwtsError) as e:
                ctx.unpack(bad, out=out)
            assert e.value.code == code and (out == 0x5A).all(), name
    # a member read of members whose streams are sound does not see the damage elsewhere
    by_name = {name: bad for name, bad, _ in cases}
    b.upload(_u8(by_name["width 4 rewritten to 2"]))
    idx = np.array([3, 1, 2], dtype=np.uint64)
    total = 9 + 4096 + 100
    assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, len(f), idx.ctypes.data, 3, c.ptr, total, ctypes.byref(got)) == 0
    assert c.download(total).tobytes() == x[8292:] + x[4096:8192] + x[8192:8292]
    # a header n beyond out_cap, and the context still works afterwards
    b.upload(_u8(f))
    assert pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(f), c.ptr, n - 1, ctypes.byref(got)) == E_SPACE
    assert ctx.unpack_device(b, len(f), c, n) == n and c.download(n).tobytes() == x
    out = np.full(n - 1, 0x5A, dtype=np.uint8)
    with pytest.raises(pkg.BwtsError) as e:
        ctx.unpack(f, out=out)
    assert e.value.code == E_SPACE and (out == 0x5A).all()
    # a frame of the other magic has no members
    v2 = P2.pack(x, 4096)
    b.upload(_u8(v2))
    c.upload(np.full(64, MARK, dtype=np.uint8))
    assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, len(v2), every.ctypes.data, 1, c.ptr, n, ctypes.byref(got)) == E_FORMAT
    assert (c.download(64) == MARK).all()
    with pytest.raises(pkg.BwtsError) as e:
        ctx.unpack_members(v2, [0])
    assert e.value.code == E_FORMAT


def test_capacity(pkg, ctx, bufs, reference):
    """Exact capacity packs; one byte, or 16, short of the frame is BWTS_E_SPACE with nothing written at all."""
    a, b, c = bufs
    members, widths, x, want = reference
    a.upload(x)
    size = want.size
    ls, ws = np.array(C.LENGTHS, dtype=np.uint64), np.array(widths, dtype=np.uint32)
    mark = np.full(size + 64, MARK, dtype=np.uint8)
    b.upload(mark)
    assert ctx.pack_members_device(a, C.LENGTHS, widths, b, size) == size
    assert np.array_equal(b.download(size + 64), np.concatenate((want, mark[size:])))
    got = ctypes.c_uint64(0)
    for short in (1, 16, size - 32 - 32 * len(C.LENGTHS)):
        b.upload(mark)
        rc = pkg.lib().bwts_pack_members_device(ctx._h, a.ptr, ls.ctypes.data, ws.ctypes.data, ls.size, b.ptr, size - short, ctypes.byref(got))
        assert rc == E_SPACE, (short, rc)
        assert np.array_equal(b.download(size + 64), mark), "BWTS_E_SPACE, but something was written"
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members(members, widths, out_cap=size - 1)
    assert e.value.code == E_SPACE


def test_arguments(pkg, ctx, bufs):
    a, b, c = bufs
    L, h = pkg.lib(), ctx._h
    got = ctypes.c_uint64(0)
    kept = []

    def arr(*v, dtype=np.uint64):
        kept.append(np.array(v, dtype=dtype))
        return kept[-1].ctypes.data

    def ws(*v):
        return arr(*v, dtype=np.uint32)

    cap = 1 << 16
    fn = L.bwts_pack_members_device
    assert fn(h, a.ptr, arr(3000, 2000), ws(4, 1), 2, b.ptr, cap, ctypes.byref(got)) == 0
    for w in (0, 3, 16, 0x10004):
        assert fn(h, a.ptr, arr(3000, 2000), ws(4, w), 2, b.ptr, cap, ctypes.byref(got)) == E_ARG, w
    assert fn(None, a.ptr, arr(3000, 2000), None, 2, b.ptr, cap, ctypes.byref(got)) == E_ARG and fn(h, None, arr(3000, 2000), None, 2, b.ptr, cap, ctypes.byref(got)) == E_ARG
    assert fn(h, a.ptr, None, None, 2, b.ptr, cap, ctypes.byref(got)) == E_ARG and fn(h, a.ptr, arr(3000, 2000), None, 2, None, cap, ctypes.byref(got)) == E_ARG
    assert fn(h, a.ptr, arr(3000, 2000), None, 2, b.ptr, cap, None) == E_ARG and fn(h, a.ptr, arr(3000, 2000), None, 0, b.ptr, cap, ctypes.byref(got)) == E_ARG
    assert fn(h, a.ptr, arr(3000, 0), None, 2, b.ptr, cap, ctypes.byref(got)) == E_ARG
    assert fn(h, a.ptr, arr(3000, 2000), None, 2, b.ptr + 8, cap, ctypes.byref(got)) == E_ARG           # d_out off 16 bytes
    assert fn(h, a.ptr, arr(3000, 2000), None, 2, a.ptr + 4992, cap, ctypes.byref(got)) == E_ARG        # overlap
    assert fn(h, a.ptr, arr(1 << 32, 1), None, 2, b.ptr, cap, ctypes.byref(got)) == E_RANGE             # decided before the data is touched
    assert fn(h, a.ptr, arr(1, 1), None, (1 << 20) + 1, b.ptr, cap, ctypes.byref(got)) == E_RANGE
    assert fn(h, a.ptr, arr(3000, 2000), None, 2, b.ptr, 32 + 64 + 31, ctypes.byref(got)) == E_SPACE
    host = np.zeros(64, dtype=np.uint8).ctypes.data
    assert L.bwts_pack_members(h, host, arr(16), ws(3), 1, host, 64, ctypes.byref(got)) == E_ARG
    assert L.bwts_pack_members(h, None, arr(16), None, 1, host, 64, ctypes.byref(got)) == E_ARG
    assert L.bwts_pack_members(h, host, arr(1 << 32, 1), None, 2, host, 64, ctypes.byref(got)) == E_RANGE
    with pytest.raises(pkg.BwtsError):
        ctx.pack_members([b"abc", b"de"], [2])


def test_one_member(pkg, ctx, bufs):
    """count == 1 goes through the single-input stages: the bytes are the model's all the same."""
    a, b, c = bufs
    for ln, w in ((1, 8), (7, 4), (4097, 1), (8193, 2), (32775, 8), (70001, 4)):
        x = fixture_input(ln, ln) if w == 1 else _u8(MM.P3.f32_field(-(-ln // 4), seed=ln)[:ln]).tobytes()
        want = _u8(MM.pack([x], [w]))
        a.upload(_u8(x))
        size = ctx.pack_members_device(a, [ln], [w], b, pkg.pack_members_bound([ln]))
        y = b.download(size)
        assert size == want.size and np.array_equal(y, want), "one member of %d at %d: %s" % (ln, w, _first_diff(y, want))
        c.upload(np.full(ln + 64, MARK, dtype=np.uint8))
        assert ctx.unpack_device(b, size, c, ln) == ln
        got = c.download(ln + 64)
        assert got[:ln].tobytes() == x and (got[ln:] == MARK).all()
        assert ctx.unpack_members(want, [0, 0]) == [x, x]
        assert ctx.debug_unpack_ranges_report()["single"]


def test_width_1_members_of_one_length_are_version_2s_streams(pkg, ctx, bufs):
    """Members of width 1 and one length 4096: the streams of the version-2 "BWTZ" frame at B = 4096 of the same bytes; header, width
    word and length word alone differ."""
    a, b, c = bufs
    x = _u8(fixture_input(5 * 4096, 33))
    a.upload(x)
    ls = [4096] * 5
    size = ctx.pack_members_device(a, ls, None, b, pkg.pack_members_bound(ls))
    f = b.download(size).tobytes()
    v2 = ctx.pack_device(a, x.size, 4096, b, pkg.pack_bound(x.size, 4096, version=2), version=2)
    g = b.download(v2).tobytes()
    fixed = 32 + 32 * 5
    assert f == MM.pack([x[k:k + 4096].tobytes() for k in range(0, x.size, 4096)]) and g == P2.pack(x.tobytes(), 4096)
    assert size == v2 and f[fixed:] == g[fixed:] and f[:4] == b"BWTM" and g[:4] == b"BWTZ"
    for k in range(5):
        e, e2 = f[32 + 32 * k:64 + 32 * k], g[32 + 32 * k:64 + 32 * k]
        assert e[:12] == e2[:12] and e[16:24] == e2[16:24] and e[12:16] == b"\x01\0\0\0" and e2[12:16] == bytes(4)


def test_golden_fixtures_on_the_device(pkg, ctx, bufs):
    a, b, c = bufs
    for name, (members, widths) in C.fixtures().items():
        f = _u8(open(os.path.join(GOLDEN, name), "rb").read())
        x = b"".join(members)
        b.upload(f)
        c.upload(np.zeros(len(x), dtype=np.uint8))
        assert ctx.unpack_device(b, f.size, c, len(x)) == len(x) and c.download(len(x)).tobytes() == x, name
        a.upload(_u8(x))
        ls = [len(m) for m in members]
        assert ctx.pack_members_device(a, ls, widths, b, f.size) == f.size and np.array_equal(b.download(f.size), f), name
        assert pkg.frame_members(f) == (ls, widths)


def test_cli_unpack_reads_member_frames(tmp_path):
    """bwts_unpack steps through frames with bwts_unpack_size and unpacks each: a member frame, then a "BWTZ" frame behind it, and a
    range across the two."""
    from test_pack_gpu import _run
    members, _ = C.small_set()
    x = b"".join(members)
    tail = fixture_input(5000, 44)
    packed, back = tmp_path / "members.bwz", tmp_path / "members.out"
    packed.write_bytes(open(os.path.join(GOLDEN, "members_four_mixed.bin"), "rb").read() + P2.pack(tail))
    r = _run("bwts_unpack", packed, back)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert back.read_bytes() == x + tail
    r = _run("bwts_unpack", "-r", "%d:%d" % (4090, 10), "-r", "%d:%d" % (len(x) - 3, 6), packed, back)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert back.read_bytes() == x[4090:4100] + x[-3:] + tail[:3]
