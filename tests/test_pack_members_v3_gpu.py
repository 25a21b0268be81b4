"""GPU suite of version 3 of the member frame (include/bwts_members.h), through the C-ABI: the device's frame byte for byte against the
CPU model (tests/pack_members_v3_model.py) and bwts_unpack_device back to the input at every size where the cut of a direct member,
the coder's tiles and blocks or the mix of chain and direct members takes another path; the readers; the refusals that version 3
adds; what a pack keeps on the device."""
import ctypes

import numpy as np
import pytest

import members_v3_cases as C3
import pack_members_model as MM
import pack_members_v2_model as M2
import pack_members_v3_model as M3
from test_pack_gpu import _first_diff, _u8

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
MARK = 0xA5
BIG = 4096 * 4096           # the largest case: 4096 members of 4 KiB
P = 8192                    # the plane minimum


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame, as large as the bound of the largest case; c: output"""
    a, c = ctx.alloc(BIG + 256), ctx.alloc(BIG + 256)
    b = ctx.alloc(pkg.pack_members_bound([4096] * 4096, [2] * 4096, [1] * 4096) + 256)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def arrays(spec):
    ls = np.array([s[0] for s in spec], dtype=np.uint64)
    ws, fs, ms = (np.array([s[i] for s in spec], dtype=np.uint32) for i in (1, 2, 3))
    return ls, ws, fs, ms


def device_pack(pkg, ctx, bufs, spec, x, cap=None, methods=True):
    """bwts_pack_members_m_device of the members of spec that lie in x: (rc, the frame's bytes)"""
    a, b, c = bufs
    ls, ws, fs, ms = arrays(spec)
    a.upload(_u8(x))
    cap = int(pkg.lib().bwts_pack_members_bound_m(ls.ctypes.data, ws.ctypes.data, ms.ctypes.data, ls.size)) if cap is None else cap
    got = ctypes.c_uint64(0)
    rc = pkg.lib().bwts_pack_members_m_device(ctx._h, a.ptr, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ms.ctypes.data if methods else None, ls.size,
                                              b.ptr, cap, ctypes.byref(got))
    return rc, got.value


def round_trip(pkg, ctx, bufs, spec, seed, name):
    """The device's frame is the model's, and bwts_unpack_device gives the input back."""
    a, b, c = bufs
    members, widths, filters, methods = C3.make_set(spec, seed)
    x = b"".join(members)
    want = _u8(M3.pack(members, widths, filters, methods))
    rc, size = device_pack(pkg, ctx, bufs, spec, x)
    assert rc == 0 and size == want.size, (name, rc, size, want.size)
    y = b.download(size)
    assert np.array_equal(y, want), "%s: pack: %s" % (name, _first_diff(y, want))
    c.upload(np.full(len(x) + 64, MARK, dtype=np.uint8))
    got = ctypes.c_uint64(0)
    assert pkg.lib().bwts_unpack_device(ctx._h, b.ptr, size, c.ptr, len(x), ctypes.byref(got)) == 0 and got.value == len(x), name
    back = c.download(len(x) + 64)
    assert back[:len(x)].tobytes() == x and (back[len(x):] == MARK).all(), "%s: unpack: %s" % (name, _first_diff(back[:len(x)], _u8(x)))
    return want


# ---- group 1: the device's frames are the model's ----
@pytest.mark.parametrize("w", [2, 4, 8])
def test_plane_minimum(pkg, ctx, bufs, w):
    """One element short of separate planes, exactly there, and there with the longest tail."""
    for ln in (w * P - 1, w * P, w * P + (w - 1)):
        f = round_trip(pkg, ctx, bufs, [(ln, w, 0, 1)], 20 + w, "len %d at width %d" % (ln, w))
        assert struct_ext(f) == (1, w if ln >= w * P else 0)


def struct_ext(f):
    return int(f[16:20].view("<u4")[0]), int(f[20:24].view("<u4")[0])


@pytest.mark.parametrize("q", [16384, 16385, 262145])
def test_tile_and_block_edges_of_a_plane(pkg, ctx, bufs, q):
    """A plane of whole coder tiles, of one byte more, and of one byte more than a coder block: the next plane begins a new stream."""
    round_trip(pkg, ctx, bufs, [(2 * q, 2, 0, 1)], 30, "q = %d" % q)


def test_small_and_filtered_direct_members(pkg, ctx, bufs):
    for name, spec in (("width 1", [(70001, 1, 0, 1)]), ("len < w", [(3, 4, 0, 1)]), ("len < w among others", [(5, 8, 0, 1), (4096, 1, 0, 0), (1, 2, 0, 1)]),
                       ("filter and planes", [(4 * P + 2, 4, 1, 1)]), ("filter, one segment", [(8 * 300, 8, 1, 1), (9000, 2, 1, 1)])):
        round_trip(pkg, ctx, bufs, spec, 40, name)


def test_member_patterns(pkg, ctx, bufs):
    rng = np.random.default_rng(9)
    alternating = [(int(rng.integers(4096, 40961)), int(rng.choice([1, 2, 4, 8])), 0, k & 1) for k in range(64)]
    for name, spec in (
            ("a single direct member with planes", [(2 * P + 1, 2, 0, 1)]),
            ("all direct", [(2 * P + 1, 2, 0, 1), (5000, 4, 0, 1), (8 * P, 8, 0, 1), (77, 1, 0, 1)]),
            ("direct first and last", [(4 * P + 3, 4, 0, 1), (4096, 1, 0, 0), (9001, 2, 0, 0), (2 * P, 2, 0, 1)]),
            ("chain first and last", [(4096, 2, 0, 0), (4 * P + 3, 4, 0, 1), (6000, 2, 0, 1), (5000, 1, 0, 0)]),
            ("one chain member between direct ones", [(6000, 2, 0, 1), (5000, 1, 0, 0), (2 * P + 1, 2, 0, 1)]),
            ("strict alternation over 64 members", alternating)):
        round_trip(pkg, ctx, bufs, spec, 50, name)


def test_4096_direct_members(pkg, ctx, bufs):
    round_trip(pkg, ctx, bufs, [(4096, 2, 0, 1)] * 4096, 1000, "4096 direct members of 4 KiB")


def test_golden_frame(pkg, ctx, bufs):
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", C3.GOLDEN), "rb") as h:
        golden = h.read()
    members, widths, filters, methods = C3.golden_set()
    rc, size = device_pack(pkg, ctx, bufs, C3.GOLDEN_MEMBERS, b"".join(members))
    assert rc == 0 and bufs[1].download(size).tobytes() == golden
    assert ctx.unpack(golden).tobytes() == b"".join(members)


def test_no_method_is_the_earlier_frame(pkg, ctx, bufs):
    a, b, c = bufs
    spec = [(5000, 2, 1, 0), (4096, 1, 0, 0), (2 * P + 1, 2, 0, 0), (100, 4, 1, 0)]
    members, widths, filters, _ = C3.make_set(spec, 60)
    x = b"".join(members)
    ls, ws, fs, ms = arrays(spec)
    got = ctypes.c_uint64(0)
    a.upload(_u8(x))
    cap = pkg.pack_members_bound(ls)
    assert pkg.lib().bwts_pack_members_f_device(ctx._h, a.ptr, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ls.size, b.ptr, cap, ctypes.byref(got)) == 0
    want = b.download(got.value).tobytes()
    assert want == M2.pack(members, widths, filters)
    for methods in (False, True):       # (methods == NULL, and methods all 0)
        rc, size = device_pack(pkg, ctx, bufs, spec, x, methods=methods)
        assert rc == 0 and b.download(size).tobytes() == want
    assert int(pkg.lib().bwts_pack_members_bound_m(ls.ctypes.data, ws.ctypes.data, None, ls.size)) == cap


def test_capacity(pkg, ctx, bufs):
    """The bound packs; exactly the frame's size packs; 16 bytes short of it is BWTS_E_SPACE with nothing written at all."""
    a, b, c = bufs
    spec = [(2 * P + 1, 2, 0, 1), (5000, 1, 0, 0), (4 * P, 4, 0, 1), (300, 8, 0, 1)]
    members, widths, filters, methods = C3.make_set(spec, 70)
    x = b"".join(members)
    want = _u8(M3.pack(members, widths, filters, methods))
    bound = pkg.pack_members_bound([s[0] for s in spec], widths, methods)
    assert bound == M3.bound([s[0] for s in spec], widths, methods) and want.size <= bound
    mark = np.full(want.size + 64, MARK, dtype=np.uint8)
    for cap in (bound, want.size):
        b.upload(mark)
        rc, size = device_pack(pkg, ctx, bufs, spec, x, cap=cap)
        assert rc == 0 and np.array_equal(b.download(want.size + 64), np.concatenate((want, mark[want.size:]))), cap
    b.upload(mark)
    rc, _ = device_pack(pkg, ctx, bufs, spec, x, cap=want.size - 16)
    assert rc == E_SPACE and np.array_equal(b.download(want.size + 64), mark), "BWTS_E_SPACE, but something was written"
    # incompressible direct members at exactly the bound: the coder never needs more
    noise = [np.random.default_rng(k).integers(0, 256, ln, dtype=np.uint8).tobytes() for k, ln in enumerate((2 * P + 1, 4097))]
    nspec = [(2 * P + 1, 2, 0, 1), (4097, 1, 0, 1)]
    rc, size = device_pack(pkg, ctx, bufs, nspec, b"".join(noise))
    assert rc == 0 and b.download(size).tobytes() == M3.pack(noise, [2, 1], None, [1, 1])
    # a method that is neither, with the bad widths
    ls, ws, fs, ms = arrays(spec)
    bad = ms.copy()
    bad[1] = 2
    got = ctypes.c_uint64(0)
    L = pkg.lib()
    assert L.bwts_pack_members_m_device(ctx._h, a.ptr, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, bad.ctypes.data, ls.size, b.ptr, bound, ctypes.byref(got)) == E_ARG
    assert int(L.bwts_pack_members_bound_m(ls.ctypes.data, ws.ctypes.data, bad.ctypes.data, ls.size)) == 0


# ---- group 2: the readers ----
READ_SPEC = [(20000, 2, 0, 1), (5000, 1, 0, 0), (2 * P + 6, 2, 0, 1), (4096, 4, 1, 0), (9000, 4, 1, 1), (3000, 1, 0, 0), (4 * P + 1, 4, 0, 1)]


@pytest.fixture(scope="module")
def read_set():
    """The readers' member set, its concatenation and the model's frame: made once, shared, left unchanged."""
    members, widths, filters, methods = C3.make_set(READ_SPEC, 80)
    return members, widths, filters, methods, b"".join(members), _u8(M3.pack(members, widths, filters, methods))


def test_ranges(pkg, ctx, bufs, read_set):
    a, b, c = bufs
    members, widths, filters, methods, x, f = read_set
    off = np.concatenate(([0], np.cumsum([s[0] for s in READ_SPEC]))).tolist()
    b.upload(f)
    sets = [
        ("direct members alone", [(off[0] + 7, 300), (off[2] + P - 3, 9), (off[6], 5)], {"zrl", "mtf", "inverse", "regroup"}, set()),
        ("one direct member with planes", [(off[2] + 1, 2 * P)], {"zrl", "mtf", "inverse", "regroup"}, set()),
        ("chain members alone", [(off[1] + 5, 10), (off[5], 3000)], {"regroup"}, {"zrl", "mtf", "inverse"}),
        ("across a seam either way", [(off[1] - 4, 8), (off[4] - 1, 2)], set(), {"zrl", "mtf", "inverse", "regroup", "delta", "join"}),
        ("whole input", [(0, len(x))], set(), {"zrl", "mtf", "inverse", "regroup"}),
    ]
    for name, rs, absent, present in sets:
        total = sum(nb for _, nb in rs)
        c.upload(np.full(total + 64, MARK, dtype=np.uint8))
        assert ctx.unpack_ranges_device(b, f.size, rs, c, total) == total, name
        got = c.download(total + 64)
        assert got[:total].tobytes() == b"".join(x[o:o + nb] for o, nb in rs) and (got[total:] == MARK).all(), name
        stages = set(ctx.debug_unpack_ranges_report()["stages"])
        assert not stages & absent and stages >= present | {"decode", "crc", "cut"}, (name, stages)
    # the host form, once
    rs = sets[3][1]
    assert [g.tobytes() for g in ctx.unpack_ranges(f, rs)] == [x[o:o + nb] for o, nb in rs] == M3.unpack_ranges(f.tobytes(), rs)


def test_members_and_frame_members(pkg, ctx, bufs, read_set):
    a, b, c = bufs
    members, widths, filters, methods, x, f = read_set
    b.upload(f)
    perm = np.array([6, 0, 3, 6, 2, 1, 2], dtype=np.uint64)
    total = sum(READ_SPEC[k][0] for k in perm.tolist())
    c.upload(np.full(total + 64, MARK, dtype=np.uint8))
    got = ctypes.c_uint64(0)
    assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, f.size, perm.ctypes.data, perm.size, c.ptr, total, ctypes.byref(got)) == 0 and got.value == total
    back = c.download(total + 64)
    assert back[:total].tobytes() == b"".join(members[k] for k in perm.tolist()) and (back[total:] == MARK).all()
    assert ctx.debug_unpack_ranges_report()["blocks"] == 5
    n = len(READ_SPEC)
    ls, ws, fs, ms = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert pkg.lib().bwts_frame_members_m(f.ctypes.data, f.size, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ms.ctypes.data, n, ctypes.byref(got)) == 0
    assert got.value == n and (ls.tolist(), ws.tolist(), fs.tolist(), ms.tolist()) == ([s[0] for s in READ_SPEC], widths, filters, methods)
    assert pkg.lib().bwts_frame_members_m(f.ctypes.data, f.size, None, None, None, ms.ctypes.data, n - 1, ctypes.byref(got)) == E_SPACE
    # the host forms and the Python wrappers, once each
    assert ctx.unpack_members(f, [4, 2]) == [members[4], members[2]]
    assert pkg.frame_members(f) == ([s[0] for s in READ_SPEC], widths) and pkg.frame_member_filters(f) == filters and pkg.frame_member_methods(f) == methods
    g = ctx.pack_members(members, widths, filters, methods=methods)
    assert np.array_equal(g, f) and ctx.unpack(g).tobytes() == x and pkg.unpack_size(g) == (len(x), g.size)
    a.upload(_u8(x))
    size = ctx.pack_members_device(a, [s[0] for s in READ_SPEC], widths, b, pkg.pack_members_bound([s[0] for s in READ_SPEC], widths, methods), filters=filters,
                                   methods=methods)
    assert size == f.size and np.array_equal(b.download(size), f)
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members(members[:2], widths[:2], None, methods=[1, 2])
    assert e.value.code == E_ARG


# ---- group 3: untrusted input ----
def test_malformed_version_3_frames(pkg, ctx, bufs):
    a, b, c = bufs
    x, f, cases = C3.malformed_cases()
    n = len(x)
    got = ctypes.c_uint64(0)
    for name, bad, code in [("valid", f, 0)] + cases:
        b.upload(_u8(bad))
        c.upload(np.full(n + 64, MARK, dtype=np.uint8))
        rc = pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(bad), c.ptr, n, ctypes.byref(got))
        if code is None:
            # canonical still: decoded in bounds through the other cut or the other stages, never a wrong byte with BWTS_OK
            assert rc in (E_FORMAT, E_CHECKSUM), "%s: %d" % (name, rc)
            assert (c.download(n + 64)[n:] == MARK).all(), name
        else:
            assert rc == code, "%s: %d, the model says %d" % (name, rc, code)
        if code == 0:
            assert c.download(n).tobytes() == x
        if code == E_FORMAT:
            assert (c.download(n + 64) == MARK).all(), "%s: refused, but something was written" % name
    # a member that a rewritten method bit does not touch is read as before
    by_name = {name: bad for name, bad, _ in cases}
    bad = by_name["a method bit cleared, others left"]
    b.upload(_u8(bad))
    idx = np.array([3, 1], dtype=np.uint64)
    want = x[-2400:] + x[3000:3000 + 2 * P + 1]
    assert pkg.lib().bwts_unpack_members_device(ctx._h, b.ptr, len(bad), idx.ctypes.data, 2, c.ptr, len(want), ctypes.byref(got)) == 0
    assert c.download(len(want)).tobytes() == want
    # the context still works
    b.upload(_u8(f))
    assert ctx.unpack_device(b, len(f), c, n) == n and c.download(n).tobytes() == x


# ---- what a pack keeps ----
def test_memory_kept(pkg):
    """A direct member takes no arena of the transform: device_bytes after an all-direct pack of 1 MiB is below that of the method-0 pack
    of the same members, and so is that of a pack with one chain member of 4 KiB beside a direct one of 1 MiB - 4 KiB (the arena is
    sized for the chain set, not for n)."""
    n = 1 << 20
    x = _u8(C3.weights(n, 2, 90))
    cases = [([n // 4] * 4, [1] * 4), ([n // 4] * 4, [0] * 4), ([4096, n - 4096], [0, 1])]
    kept = []
    for lengths, methods in cases:
        widths = [2] * len(lengths)
        with pkg.Context(0) as c:
            a, s = c.alloc(n), c.alloc(pkg.pack_members_bound(lengths, widths, methods))
            a.upload(x)
            size = c.pack_members_device(a, lengths, widths, s, s.nbytes, methods=methods)
            kept.append(c.timings().device_bytes)
            assert pkg.frame_member_methods(s.download(size)) == methods
    print("device_bytes: all direct %d, all chain %d, 4 KiB chain beside direct %d" % tuple(kept))
    assert kept[0] < kept[1] and kept[2] < kept[1], kept
