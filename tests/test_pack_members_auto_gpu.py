"""GPU suite of the estimate and of the pack that chooses (include/bwts_members.h, "The estimate", "AUTO").  The estimator against
tests/estimate_model.py with exact equality at every element count where the kernel takes another path, with and without a tail,
behind odd-length members, on the contended path (one value repeated), on differences that wrap and across a unit boundary.  The auto
pack on the eleven inputs of DESIGN section 21 and on members either side of the plane minimum: the choices and the frame are the
model's, the frame is bwts_pack_members_m_device's of the resolved arrays, and every reader takes it; the capacity contract; an
all-explicit call launches what bwts_pack_members_m_device launches; what a pack keeps; the host forms."""
import ctypes
import functools

import numpy as np
import pytest

import estimate_model as EST
import members_auto_cases as C
import pack_members_auto_model as A
import pack_members_v3_model as M3
from test_pack_gpu import _first_diff, _u8

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_SPACE = -1, -5, -9
MARK = 0xA5
AUTO = A.AUTO
U = EST.UNIT
ROOM = 2 * 8 * (3 * U + 13000)      # the largest estimator call: every element count, with and without a tail, at width 8


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame; c: output"""
    a, b, c = ctx.alloc(ROOM + 256), ctx.alloc(2 << 20), ctx.alloc(2 << 20)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def walk(rng, q, w, tail):
    """q elements of width w, a random walk under noise (both filters have something to find), and `tail` bytes behind them"""
    steps = rng.integers(-300, 300, q) + (rng.integers(0, 1 << 20, q) if w > 2 else 0) * (rng.integers(0, 16, q) == 0)
    e = np.cumsum(steps).astype(np.int64).astype("<i%d" % w) if w > 1 else (np.cumsum(steps // 60) & 255).astype(np.uint8)
    return e.tobytes() + rng.integers(0, 256, tail, dtype=np.uint8).tobytes()


def device_estimate(pkg, ctx, a, members, widths, shift=0):
    """bwts_members_estimate_device of the members, laid back to back `shift` bytes behind the buffer's start"""
    x = b"".join(members)
    a.upload(np.concatenate((np.full(shift, MARK, dtype=np.uint8), _u8(x))))
    ls, ws = np.array([len(m) for m in members], dtype=np.uint64), np.array(widths, dtype=np.uint32)
    e0, e1 = np.full(ls.size, 1 << 60, dtype=np.uint64), np.full(ls.size, 1 << 60, dtype=np.uint64)
    rc = pkg.lib().bwts_members_estimate_device(ctx._h, a.ptr + shift, ls.ctypes.data, ws.ctypes.data, ls.size, e0.ctypes.data, e1.ctypes.data)
    assert rc == 0
    return e0.tolist(), e1.tolist()


def check_estimate(pkg, ctx, a, members, widths, name, shifts=(0,)):
    want = EST.estimate_members(members, widths)
    for shift in shifts:
        got = device_estimate(pkg, ctx, a, members, widths, shift)
        bad = [(k, len(members[k]), widths[k], got[0][k], want[0][k], got[1][k], want[1][k]) for k in range(len(members))
               if (got[0][k], got[1][k]) != (want[0][k], want[1][k])]
        assert not bad, "%s, shift %d: (member, len, w, none, model, delta, model) %s" % (name, shift, bad[:6])
    return want


# ---- the estimator ----
@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_estimate_at_every_element_count(pkg, ctx, bufs, w):
    """0 (len < w), 1, 15, 16, 17, a tile less one, a tile, a tile and one, a unit less one, a unit, a unit and one element; each with a
    tail of 0 and of w - 1 bytes, in one call: behind a member with an odd tail every start is odd, and a member's first element must
    see a 0, not its neighbour's last element.  The base pointer on and off a 16-byte boundary."""
    rng = np.random.default_rng(100 + w)
    members = []
    for q in (0, 1, 15, 16, 17, 4095, 4096, 4097, U - 1, U, U + 1):
        for tail in sorted({0, w - 1}):
            if q * w + tail:
                members.append(walk(rng, q, w, tail))
    want = check_estimate(pkg, ctx, bufs[0], members, [w] * len(members), "width %d" % w, shifts=(0, 1) if w < 8 else (0, 5))
    assert any(n > d + (n >> 6) for n, d in zip(*want)) and max(len(m) for m in members) == (U + 1) * w + w - 1


def test_estimate_patterns(pkg, ctx, bufs):
    rng = np.random.default_rng(7)
    for w in (1, 2, 4, 8):
        lo, hi = (1 << (8 * w - 1)).to_bytes(w, "little"), ((1 << (8 * w - 1)) - 1).to_bytes(w, "little")
        v = bytes([0x5A] * w)
        members = [
            bytes((U + 1) * w),                     # one value repeated, the contended path: both estimates are 0
            v * 4096, v * 4096 + b"\x01" * (w - 1),  # the same value again: the second member's first difference is v, not 0
            v * 17,
            (lo + hi) * ((U + 4096) // 2),          # the minimum and the maximum of the width in turn: every difference wraps
            walk(rng, U, w, 0) + rng.integers(0, 256, 5000 * w, dtype=np.uint8).tobytes(),      # a compressible unit, then noise
        ]
        want = check_estimate(pkg, ctx, bufs[0], members, [w] * len(members), "patterns at width %d" % w)
        assert (want[0][0], want[1][0]) == (0, 0) and want[0][1] == 0 and want[1][1] > 0 and want[1][2] == want[1][1]
    # a width per member, members without an element among them
    widths = [8, 1, 4, 2, 8, 4, 1, 2]
    members = [walk(rng, q, w, t) for (q, t), w in zip(((0, 7), (33, 0), (5000, 3), (U + 3, 1), (4096, 0), (0, 2), (1, 0), (4097, 1)), widths)]
    check_estimate(pkg, ctx, bufs[0], members, widths, "mixed widths", shifts=(0, 3))


def test_estimate_4096_members_of_4_bytes(pkg, ctx, bufs):
    rng = np.random.default_rng(8)
    widths = rng.choice([1, 2, 4, 8], 4096).tolist()
    members = [rng.integers(0, 4, 4, dtype=np.uint8).tobytes() for _ in widths]
    check_estimate(pkg, ctx, bufs[0], members, widths, "4096 members of 4 bytes")


def test_estimate_refusals_and_host_form(pkg, ctx, bufs):
    a = bufs[0]
    L = pkg.lib()
    ls, ws, e = np.array([8, 8], dtype=np.uint64), np.array([4, 2], dtype=np.uint32), np.zeros(2, dtype=np.uint64)
    args = lambda lens=ls, wid=ws, cnt=2, e0=e, e1=e: (ctx._h, a.ptr, lens.ctypes.data, wid.ctypes.data, cnt, e0.ctypes.data, e1.ctypes.data)
    assert L.bwts_members_estimate_device(*args()) == 0
    assert L.bwts_members_estimate_device(*args(cnt=0)) == E_ARG
    assert L.bwts_members_estimate_device(*args(lens=np.array([8, 0], dtype=np.uint64))) == E_ARG
    assert L.bwts_members_estimate_device(*args(wid=np.array([4, 3], dtype=np.uint32))) == E_ARG
    assert L.bwts_members_estimate_device(*args(lens=np.array([1 << 32, 1], dtype=np.uint64))) == E_RANGE
    assert L.bwts_members_estimate_device(ctx._h, a.ptr, ls.ctypes.data, ws.ctypes.data, 2, None, e.ctypes.data) == E_ARG
    assert L.bwts_members_estimate_device(ctx._h, None, ls.ctypes.data, ws.ctypes.data, 2, e.ctypes.data, e.ctypes.data) == E_ARG
    # widths == NULL: every member at width 1; and the host form, through the wrappers
    members = [C.inputs()[0][:9001], C.inputs()[6][:5000], C.inputs()[5][:8 * 1000 + 3]]
    assert ctx.members_estimate(members) == EST.estimate_members(members)
    assert ctx.members_estimate(members, [4, 1, 8]) == EST.estimate_members(members, [4, 1, 8])
    a.upload(_u8(b"".join(members)))
    assert ctx.members_estimate_device(a, [len(m) for m in members], [4, 1, 8]) == EST.estimate_members(members, [4, 1, 8])


# ---- the pack that chooses ----
@functools.lru_cache(maxsize=None)
def auto_set():
    """The eleven inputs, and the two of width 2 cut to one element less than the plane minimum, to it, and to one more: (members, widths)"""
    members, widths = list(C.inputs()), list(C.WIDTHS)
    for k in (1, 4):
        for ln in (16384 - 2, 16384, 16384 + 2):
            members.append(C.inputs()[k][:ln])
            widths.append(2)
    return members, widths


def device_auto(pkg, ctx, bufs, members, widths, filters, methods, cap=None):
    """bwts_pack_members_a_device: (rc, size, filters_out, methods_out)"""
    a, b, c = bufs
    a.upload(_u8(b"".join(members)))
    ls, ws = np.array([len(m) for m in members], dtype=np.uint64), np.array(widths, dtype=np.uint32)
    fs, ms = np.array(filters, dtype=np.uint32), np.array(methods, dtype=np.uint32)
    fo, mo = np.full(ls.size, 99, dtype=np.uint32), np.full(ls.size, 99, dtype=np.uint32)
    cap = int(pkg.lib().bwts_pack_members_bound_a(ls.ctypes.data, ws.ctypes.data, ms.ctypes.data, ls.size)) if cap is None else cap
    got = ctypes.c_uint64(0)
    rc = pkg.lib().bwts_pack_members_a_device(ctx._h, a.ptr, ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ms.ctypes.data, ls.size, b.ptr, cap,
                                              ctypes.byref(got), fo.ctypes.data, mo.ctypes.data)
    return rc, got.value, fo.tolist(), mo.tolist()


def checked_auto(pkg, ctx, bufs, members, widths, filters, methods, name):
    """The choices and the frame are the model's; the frame is bwts_pack_members_m_device's of the resolved arrays; unpack restores the
    input and writes nothing behind it.  Returns the frame."""
    a, b, c = bufs
    x = b"".join(members)
    fs, ms = A.resolve(members, widths, filters, methods)
    want = _u8(M3.pack(members, widths, fs, ms))
    rc, size, fo, mo = device_auto(pkg, ctx, bufs, members, widths, filters, methods)
    assert rc == 0 and (fo, mo) == (fs, ms), (name, rc, fo, fs, mo, ms)
    y = b.download(size)
    assert np.array_equal(y, want), "%s: auto pack: %s" % (name, _first_diff(y, want))
    lengths = [len(m) for m in members]
    size_m = ctx.pack_members_device(a, lengths, widths, b, pkg.pack_members_bound(lengths, widths, ms), filters=fs, methods=ms)
    assert np.array_equal(b.download(size_m), want), "%s: explicit pack: %s" % (name, _first_diff(b.download(size_m), want))
    c.upload(np.full(len(x) + 64, MARK, dtype=np.uint8))
    assert ctx.unpack_device(b, size_m, c, len(x)) == len(x), name
    back = c.download(len(x) + 64)
    assert back[:len(x)].tobytes() == x and (back[len(x):] == MARK).all(), "%s: unpack: %s" % (name, _first_diff(back[:len(x)], _u8(x)))
    return want


def test_auto_single_members(pkg, ctx, bufs):
    members, widths = auto_set()
    for k, (m, w) in enumerate(zip(members, widths)):
        f = checked_auto(pkg, ctx, bufs, [m], [w], [AUTO], [AUTO], "member %d" % k)
        if k < 11:
            assert (pkg.frame_member_filters(f), pkg.frame_member_methods(f)) == ([C.FILTERS[k]], [C.METHODS[k]]), C.NAMES[k]


def test_auto_mixed_call_and_readers(pkg, ctx, bufs):
    a, b, c = bufs
    members, widths = auto_set()
    n = len(members)
    f = checked_auto(pkg, ctx, bufs, members, widths, [AUTO] * n, [AUTO] * n, "all seventeen")
    assert pkg.frame_member_filters(f)[:11] == C.FILTERS and pkg.frame_member_methods(f)[:11] == C.METHODS
    # either side of the plane minimum the direct candidate is one stream, then two: the choice is the model's on both sides
    assert [M3.table_words(len(m), 2, 1) for m in members[11:]] == [0, 2, 2, 0, 2, 2]
    # the readers take the frame as any other: whole members in any order, and ranges across a seam between the two methods
    x = b"".join(members)
    off = np.concatenate(([0], np.cumsum([len(m) for m in members]))).tolist()
    b.upload(f)
    idx = [16, 3, 0, 11]
    total = sum(len(members[k]) for k in idx)
    c.upload(np.full(total + 64, MARK, dtype=np.uint8))
    assert ctx.unpack_members_device(b, f.size, idx, c, total) == total
    back = c.download(total + 64)
    assert back[:total].tobytes() == b"".join(members[k] for k in idx) and (back[total:] == MARK).all()
    rs = [(off[3] - 5, 10), (off[6] + 100, 3000), (off[12] - 1, 2), (off[17] - 7, 7)]
    total = sum(nb for _, nb in rs)
    c.upload(np.full(total + 64, MARK, dtype=np.uint8))
    assert ctx.unpack_ranges_device(b, f.size, rs, c, total) == total
    back = c.download(total + 64)
    assert back[:total].tobytes() == b"".join(x[o:o + nb] for o, nb in rs) and (back[total:] == MARK).all()


def test_auto_beside_explicit_values(pkg, ctx, bufs):
    """Half the members carry explicit values, in every pairing with AUTO; explicit values pass through, also where the rules would
    have chosen otherwise."""
    members, widths = auto_set()
    n = len(members)
    filters = [(AUTO, 0, 1, AUTO)[k % 4] for k in range(n)]
    methods = [(AUTO, AUTO, 1, 0, 0, 1)[k % 6] for k in range(n)]
    f = checked_auto(pkg, ctx, bufs, members, widths, filters, methods, "half explicit")
    got_f, got_m = pkg.frame_member_filters(f), pkg.frame_member_methods(f)
    assert all(g == v for g, v in zip(got_f, filters) if v != AUTO) and all(g == v for g, v in zip(got_m, methods) if v != AUTO)
    # filters alone open, one method for all: the frames of version 2 and of version 3 without a chain member
    for md in (0, 1):
        checked_auto(pkg, ctx, bufs, members[:6], widths[:6], [AUTO] * 6, [md] * 6, "filters open, method %d" % md)
    # methods alone open, and a single chain candidate beside direct members (the single-input chain stages)
    checked_auto(pkg, ctx, bufs, members[:6], widths[:6], [0, 1, 0, 1, 1, 0], [AUTO] * 6, "methods open")
    checked_auto(pkg, ctx, bufs, members[2:5], widths[2:5], [0, AUTO, 1], [1, AUTO, 1], "one candidate of both kinds")


def test_auto_capacity_and_refusals(pkg, ctx, bufs):
    """The bound packs; exactly the frame's size packs; one byte less is BWTS_E_SPACE with nothing written at all."""
    a, b, c = bufs
    members, widths = auto_set()
    members, widths = members[:5], widths[:5]
    want = _u8(A.pack(members, widths))
    lengths = [len(m) for m in members]
    bound = pkg.pack_members_bound_auto(lengths, widths)
    assert bound == A.bound(lengths, widths) and want.size <= bound
    mark = np.full(want.size + 64, MARK, dtype=np.uint8)
    for cap in (bound, want.size):
        b.upload(mark)
        rc, size, _, _ = device_auto(pkg, ctx, bufs, members, widths, [AUTO] * 5, [AUTO] * 5, cap=cap)
        assert rc == 0 and np.array_equal(b.download(want.size + 64), np.concatenate((want, mark[want.size:]))), cap
    for filters, methods in (([AUTO] * 5, [AUTO] * 5), ([AUTO] * 5, [1] * 5)):
        fs, ms = A.resolve(members, widths, filters, methods)
        size = len(M3.pack(members, widths, fs, ms))
        b.upload(mark)
        rc, _, _, _ = device_auto(pkg, ctx, bufs, members, widths, filters, methods, cap=size - 1)
        assert rc == E_SPACE and np.array_equal(b.download(want.size + 64), mark), "BWTS_E_SPACE, but something was written"
    # a filter or a method that is neither a value nor AUTO, and the calls that take no AUTO
    assert device_auto(pkg, ctx, bufs, members, widths, [AUTO, 2, 0, 0, 0], [AUTO] * 5, cap=bound)[0] == E_ARG
    assert device_auto(pkg, ctx, bufs, members, widths, [AUTO] * 5, [0, 0, 254, 0, 0], cap=bound)[0] == E_ARG
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members_device(a, lengths, widths, b, bound, filters=[AUTO] * 5, methods=[0] * 5)
    assert e.value.code == E_ARG
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members_device(a, lengths, widths, b, bound, filters=[0] * 5, methods=[AUTO] * 5)
    assert e.value.code == E_ARG


def kernels_of(ctx):
    return {name: (k["launches"], k["elems"], k["alg_bytes"]) for name, k in ctx.timings().as_dict()["kernels"].items()}


def test_an_explicit_call_launches_what_the_m_call_launches(pkg, ctx, bufs):
    a, b, c = bufs
    members, widths = auto_set()
    members, widths = members[:6], widths[:6]
    lengths = [len(m) for m in members]
    filters, methods = [1, 0, 0, 1, 1, 1], [1, 1, 0, 0, 1, 0]
    rc, size, fo, mo = device_auto(pkg, ctx, bufs, members, widths, filters, methods)
    assert rc == 0 and (fo, mo) == (filters, methods)
    f, auto_kernels = b.download(size), kernels_of(ctx)
    size_m = ctx.pack_members_device(a, lengths, widths, b, pkg.pack_members_bound(lengths, widths, methods), filters=filters, methods=methods)
    assert np.array_equal(b.download(size_m), f) and kernels_of(ctx) == auto_kernels
    # with the filters open the estimator's launch comes on top, and nothing else
    rc, size, fo, _ = device_auto(pkg, ctx, bufs, members, widths, [AUTO] * 6, methods)
    assert rc == 0
    open_kernels = kernels_of(ctx)
    size_m = ctx.pack_members_device(a, lengths, widths, b, pkg.pack_members_bound(lengths, widths, methods), filters=fo, methods=methods)
    explicit = kernels_of(ctx)
    assert open_kernels["other"][0] == explicit["other"][0] + 1 and {k: v for k, v in open_kernels.items() if k != "other"} == {k: v for k, v in explicit.items() if k != "other"}


def test_memory_kept(pkg):
    """device_bytes after a pack of direct members with the filters open stays at the all-direct figure of the explicit pack, measured
    here on the same members, but for the arena's granule (the estimator takes 16 bytes per unit from the arena, which grows in steps
    of 1 MiB); it stays below the all-chain figure, the bar of the version-3 suite's test."""
    n = 1 << 20
    x = np.random.default_rng(90).standard_normal(n // 2).astype("<f4").view("<u4") >> 16
    x = _u8(x.astype("<u2").tobytes())
    lengths, widths = [n // 4] * 4, [2] * 4
    kept = []
    for filters, methods, auto in (([0] * 4, [1] * 4, False), ([AUTO] * 4, [1] * 4, True), ([0] * 4, [0] * 4, False)):
        with pkg.Context(0) as c:
            a, s = c.alloc(n), c.alloc(pkg.pack_members_bound(lengths, widths, methods))
            a.upload(x)
            if auto:
                size, fo, mo = c.pack_members_auto_device(a, lengths, widths, s, s.nbytes, filters, methods)
                assert fo == [0] * 4 and mo == methods
            else:
                size = c.pack_members_device(a, lengths, widths, s, s.nbytes, filters=filters, methods=methods)
            kept.append(c.timings().device_bytes)
    print("device_bytes: all direct %d, filters open %d, all chain %d" % tuple(kept))
    assert kept[1] <= kept[0] + (1 << 20) and kept[1] < kept[2], kept


def test_host_forms(pkg, ctx):
    members, widths = auto_set()
    members, widths = members[:4] + members[11:13], widths[:4] + widths[11:13]
    f = ctx.pack_members_auto(members, widths)
    assert f.tobytes() == A.pack(members, widths) and ctx.unpack(f).tobytes() == b"".join(members)
    fs, ms = A.resolve(members, widths)
    assert (pkg.frame_member_filters(f), pkg.frame_member_methods(f)) == (fs, ms)
    g = ctx.pack_members_auto(members, widths, filters=0, methods=[AUTO, 1, 0, AUTO, 1, AUTO])
    assert g.tobytes() == A.pack(members, widths, 0, [AUTO, 1, 0, AUTO, 1, AUTO]) and ctx.unpack(g).tobytes() == b"".join(members)
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_members_auto(members, widths, out_cap=f.size - 16)
    assert e.value.code == E_SPACE
