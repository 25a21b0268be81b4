"""GPU suite of the member calls over tables of device pointers (include/bwts_members.h, "Pointers").  The copy between scattered
buffers (csrc/pieces.hip, scatter_pieces_kernel) through bwts_gather_device and bwts_scatter_device against numpy slicing: every pairing
of misalignments on either side, lengths around the tile, members that are whole allocations, a thousand one-byte members; gather then
scatter is the identity and no byte around a destination changes.  bwts_pack_members_p_device writes the frame of
bwts_pack_members_a_device over the concatenation, byte for byte; bwts_unpack_members_p_device writes every destination that names a
member and nothing else; every refusal with its code and with nothing written; tensor sets there and back."""
import ctypes

import numpy as np
import pytest

import members_auto_cases as CA
import members_cases as C1
import members_v3_cases as C3
import pack_members_v3_model as M3
import pack_range_model as R

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
AUTO = 255
T = R.T
CANARY = 0xC7
GUARD = 32


def noise(n, seed):
    x = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    x[x == CANARY] = 0      # a copied byte never looks like a canary
    return x


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


class Slots:
    """Members in guarded slots of one allocation: every member has at least GUARD canary bytes on both sides."""

    def __init__(self, ctx, places, nbytes):
        self.ctx, self.places, self.nbytes = ctx, list(places), nbytes        # places: (offset, bytes)
        taken = np.zeros(nbytes, dtype=bool)
        for at, b in self.places:
            assert at >= GUARD and at + b + GUARD <= nbytes and not taken[at - GUARD:at + b + GUARD].any(), "a test's slots keep their guards"
            taken[at:at + b] = True
        self.buf = ctx.alloc(nbytes)

    def image(self, members):
        img = np.full(self.nbytes, CANARY, dtype=np.uint8)
        for (at, b), m in zip(self.places, members):
            assert len(m) == b
            img[at:at + b] = u8(m)
        return img

    def fill(self, members=None):
        self.buf.upload(self.image(members) if members is not None else np.full(self.nbytes, CANARY, dtype=np.uint8))

    def ptrs(self):
        return [self.buf.ptr + at for at, _ in self.places]

    def expect(self, members, what):
        got, want = self.buf.download(self.nbytes), self.image(members)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s: first wrong byte at %d of %d" % (what, bad[0], self.nbytes)

    def free(self):
        self.buf.free()


def there_and_back(ctx, places, nbytes, seed, shift=0):
    """Members at `places` of one allocation gathered into a guarded block `shift` bytes off a 16-byte boundary, and scattered from
    there into the same places of a second allocation: the block is the concatenation, the second allocation the first, guards and all."""
    members = [noise(b, seed + k).tobytes() for k, (_, b) in enumerate(places)]
    lengths = [b for _, b in places]
    total = sum(lengths)
    src, dst = Slots(ctx, places, nbytes), Slots(ctx, places, nbytes)
    flat = ctx.alloc(total + 2 * 64 + 16)
    try:
        src.fill(members)
        dst.fill()
        flat.upload(np.full(flat.nbytes, CANARY, dtype=np.uint8))
        ctx.gather_device(src.ptrs(), lengths, flat.ptr + 64 + shift)
        got = flat.download()
        want = np.full(flat.nbytes, CANARY, dtype=np.uint8)
        want[64 + shift:64 + shift + total] = u8(b"".join(members))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "gather: first wrong byte at %d of the block (the members begin at %d)" % (bad[0], 64 + shift)
        src.expect(members, "gather wrote its sources")
        ctx.scatter_device(flat.ptr + 64 + shift, dst.ptrs(), lengths)
        dst.expect(members, "scatter")
        assert np.array_equal(flat.download(), want), "scatter wrote its source"
    finally:
        for d in (src, dst, flat):
            d.free()


# ---- the kernel through gather_device / scatter_device ----
def test_every_misalignment_pair_at_short_lengths(ctx):
    """16 x 16 misalignments x six lengths below three stores.  The scattered side's misalignment is the slot's; the contiguous side's is
    where the member falls in the block, so the members are put in an order that meets every pairing, with one-byte members between
    them where no wanted pairing begins at the block's current misalignment."""
    lengths = [1, 15, 16, 17, 31, 33]
    want = {(a, c, ln) for a in range(16) for c in range(16) for ln in lengths}
    order, at, fill = [], 0, 0
    while want:
        pick = next(((a, c, ln) for ln in lengths for a in range(16) for c in (at & 15,) if (a, c, ln) in want), None)
        if pick is None:
            pick = (fill & 15, at & 15, 1)
            fill += 1
        want.discard(pick)
        order.append((pick[0], pick[2]))
        at += pick[2]
    assert fill <= 16 * 16 * len(lengths)
    places = [(128 * k + 48 + a, ln) for k, (a, ln) in enumerate(order)]
    there_and_back(ctx, places, 128 * len(places), 1)


@pytest.mark.parametrize("a,c", [(1, 0), (0, 1), (5, 11), (0, 0)])
def test_lengths_around_the_tile(ctx, a, c):
    """One member per call (the call without a table), the scattered side `a` and the block `c` bytes off a 16-byte boundary."""
    for ln in (T - 1, T, T + 1, 2 * T + 1):
        there_and_back(ctx, [(256 + a, ln)], ln + 512 + 16, 10 + ln, shift=c)
    # ... and the four lengths in one call, a table and several tiles per member
    places, at = [], 256
    for ln in (T - 1, T, T + 1, 2 * T + 1):
        places.append((at + a, ln))
        at += (ln + a + 2 * GUARD + 255) // 256 * 256
    there_and_back(ctx, places, at + 256, 20, shift=c)


def test_members_that_are_whole_allocations(ctx):
    """5003 bytes and 1 byte in DeviceBuffers of exactly their size: both ends of every member are true ends of a buffer, and the
    aligned 16-byte pieces around them are not the member's."""
    sizes = [5003, 1, 5003, 1]
    members = [noise(b, 30 + k) for k, b in enumerate(sizes)]
    total = sum(sizes)
    src, dst = [ctx.alloc(b) for b in sizes], [ctx.alloc(b) for b in sizes]
    flat = ctx.alloc(total + 128 + 16)
    try:
        for d, m in zip(src, members):
            d.upload(m)
        for shift in (0, 7):
            flat.upload(np.full(flat.nbytes, CANARY, dtype=np.uint8))
            ctx.gather_device(src, sizes, flat.ptr + 64 + shift)
            got = flat.download()
            assert np.array_equal(got[64 + shift:64 + shift + total], np.concatenate(members))
            assert (got[:64 + shift] == CANARY).all() and (got[64 + shift + total:] == CANARY).all()
            for d in dst:
                d.upload(np.full(d.nbytes, CANARY, dtype=np.uint8))
            ctx.scatter_device(flat.ptr + 64 + shift, dst, sizes)
            for d, m in zip(dst, members):
                assert np.array_equal(d.download(), m)
        # a block that is a whole allocation too: the contiguous side ends where its buffer ends
        exact = ctx.alloc(total)
        try:
            ctx.gather_device(src, sizes, exact)
            assert np.array_equal(exact.download(), np.concatenate(members))
            ctx.scatter_device(exact, dst, sizes)
            for d, m in zip(dst, members):
                assert np.array_equal(d.download(), m)
        finally:
            exact.free()
    finally:
        for d in src + dst + [flat]:
            d.free()


def test_a_thousand_one_byte_members(ctx):
    places = [(GUARD + 33 * k, 1) for k in range(1000)]
    there_and_back(ctx, places, 33 * 1000 + 2 * GUARD, 3)
    there_and_back(ctx, places, 33 * 1000 + 2 * GUARD, 4, shift=9)


def test_gather_sources_may_overlap_and_repeat(ctx):
    x = noise(4096, 5)
    a, flat = ctx.alloc(4096), ctx.alloc(4096)
    try:
        a.upload(x)
        ptrs, lens = [a.ptr + 100, a.ptr + 100, a.ptr + 90, a.ptr + 3000], [50, 50, 100, 1096]
        ctx.gather_device(ptrs, lens, flat)
        assert np.array_equal(flat.download(sum(lens)), np.concatenate((x[100:150], x[100:150], x[90:190], x[3000:4096])))
    finally:
        a.free()
        flat.free()


def test_gather_and_scatter_refusals(pkg, ctx):
    L = pkg.lib()
    a, b = ctx.alloc(4096), ctx.alloc(4096)
    try:
        a.upload(noise(4096, 6))
        b.upload(np.full(4096, CANARY, dtype=np.uint8))
        two = np.array([100, 50], dtype=np.uint64)
        ptrs = lambda *v: np.array(v, dtype=np.uint64)
        p = ptrs(a.ptr, a.ptr + 1000)
        assert L.bwts_gather_device(ctx._h, p.ctypes.data, two.ctypes.data, 2, b.ptr) == 0
        b.upload(np.full(4096, CANARY, dtype=np.uint8))
        for name, rc, want in [
                ("no table", L.bwts_gather_device(ctx._h, None, two.ctypes.data, 2, b.ptr), E_ARG),
                ("no lengths", L.bwts_gather_device(ctx._h, p.ctypes.data, None, 2, b.ptr), E_ARG),
                ("no output", L.bwts_gather_device(ctx._h, p.ctypes.data, two.ctypes.data, 2, None), E_ARG),
                ("no members", L.bwts_gather_device(ctx._h, p.ctypes.data, two.ctypes.data, 0, b.ptr), E_ARG),
                ("a zero length", L.bwts_gather_device(ctx._h, p.ctypes.data, ptrs(100, 0).ctypes.data, 2, b.ptr), E_ARG),
                ("a sum above 2^32", L.bwts_gather_device(ctx._h, p.ctypes.data, ptrs(1 << 32, 1).ctypes.data, 2, b.ptr), E_RANGE),
                ("a NULL entry", L.bwts_gather_device(ctx._h, ptrs(a.ptr, 0).ctypes.data, two.ctypes.data, 2, b.ptr), E_ARG),
                ("a source inside the output", L.bwts_gather_device(ctx._h, ptrs(a.ptr, b.ptr + 149).ctypes.data, two.ctypes.data, 2, b.ptr), E_ARG),
                ("scatter: no table", L.bwts_scatter_device(ctx._h, a.ptr, None, two.ctypes.data, 2), E_ARG),
                ("scatter: no input", L.bwts_scatter_device(ctx._h, None, p.ctypes.data, two.ctypes.data, 2), E_ARG),
                ("scatter: a NULL entry", L.bwts_scatter_device(ctx._h, a.ptr, ptrs(0, b.ptr).ctypes.data, two.ctypes.data, 2), E_ARG),
                ("scatter: two destinations share a byte", L.bwts_scatter_device(ctx._h, a.ptr, ptrs(b.ptr, b.ptr + 99).ctypes.data, two.ctypes.data, 2), E_ARG),
                ("scatter: the same destination twice", L.bwts_scatter_device(ctx._h, a.ptr, ptrs(b.ptr, b.ptr).ctypes.data, two.ctypes.data, 2), E_ARG),
                ("scatter: a destination inside the input", L.bwts_scatter_device(ctx._h, a.ptr, ptrs(b.ptr, a.ptr + 149).ctypes.data, two.ctypes.data, 2), E_ARG)]:
            assert rc == want, name
        assert (b.download() == CANARY).all(), "a refused call wrote something"
        # touching is not sharing
        assert L.bwts_scatter_device(ctx._h, a.ptr, ptrs(b.ptr + 100, b.ptr + 200).ctypes.data, two.ctypes.data, 2) == 0
        assert L.bwts_gather_device(ctx._h, ptrs(a.ptr, b.ptr + 150).ctypes.data, two.ctypes.data, 2, b.ptr) == 0
    finally:
        a.free()
        b.free()


# ---- pack identity ----
@pytest.fixture(scope="module")
def bufs(ctx):
    """a: the members back to back; b: frame; s: bytes of the slots allocation"""
    a, b = ctx.alloc(1 << 20), ctx.alloc(2 << 20)
    yield a, b
    a.free()
    b.free()


def pack_sets():
    """(name, members, widths, filters, methods), drawn from the case lists of the member suites"""
    m1, w1 = C1.member_set()
    m3, w3, f3, d3 = C3.golden_set()
    ma, wa = list(CA.inputs()), list(CA.WIDTHS)
    return [
        ("the member suite's set, no filter, the chain", m1, w1, 0, 0),
        ("the member suite's set, AUTO", m1[:11], w1[:11], AUTO, AUTO),
        ("the version-3 golden set, explicit", m3, w3, f3, d3),
        ("four of the auto suite's inputs, AUTO", [ma[k] for k in (0, 1, 3, 6)], [wa[k] for k in (0, 1, 3, 6)], AUTO, AUTO),
        ("the same, half explicit", [ma[k] for k in (4, 5, 8, 9)], [wa[k] for k in (4, 5, 8, 9)], [AUTO, 1, 0, AUTO], [1, AUTO, AUTO, 0]),
        ("one member", [ma[1]], [2], AUTO, AUTO),
        ("members of 1 byte", [m[:1] for m in m1[:7]], [1, 2, 4, 8, 1, 2, 4], AUTO, AUTO),
        ("one member of 1 byte", [m1[0]], [1], 0, 0),
    ]


def scattered(lengths, seed):
    """Places for the members in shuffled address order, every one at an odd address"""
    order = np.random.default_rng(seed).permutation(len(lengths)).tolist()
    places, at = [None] * len(lengths), 64
    for k in order:
        places[k] = (at | 1, lengths[k])
        at = ((at | 1) + lengths[k] + 2 * GUARD + 15) // 16 * 16
    return places, at + 64


def kernels_of(ctx):
    return {name: (k["launches"], k["elems"], k["alg_bytes"]) for name, k in ctx.timings().as_dict()["kernels"].items()}


@pytest.mark.parametrize("case", range(len(pack_sets())))
def test_the_frame_is_the_contiguous_calls(pkg, ctx, bufs, case):
    a, b = bufs
    name, members, widths, filters, methods = pack_sets()[case]
    lengths = [len(m) for m in members]
    cap = pkg.pack_members_bound_auto(lengths, widths, methods)
    a.upload(u8(b"".join(members)))
    size, fo, mo = ctx.pack_members_auto_device(a, lengths, widths, b, cap, filters, methods)
    want = b.download(size)
    assert pkg.frame_members(want) == (lengths, widths)
    # (a context's first checksum makes its tables, a launch of its own: the launches are counted on a second call)
    assert ctx.pack_members_auto_device(a, lengths, widths, b, cap, filters, methods) == (size, fo, mo)
    flat_kernels = kernels_of(ctx)
    # back to back: passed on as it is, and nothing more is launched
    off = np.concatenate(([0], np.cumsum(lengths))).tolist()
    got = ctx.pack_members_ptrs_device([a.ptr + o for o in off[:-1]], lengths, widths, b, cap, filters, methods)
    assert got == (size, fo, mo) and np.array_equal(b.download(size), want), name
    assert kernels_of(ctx) == flat_kernels, name
    # scattered: shuffled address order, odd addresses
    places, room = scattered(lengths, case)
    s = Slots(ctx, places, room)
    try:
        s.fill(members)
        b.upload(np.full(size + 64, CANARY, dtype=np.uint8))
        got = ctx.pack_members_ptrs_device(s.ptrs(), lengths, widths, b, cap, filters, methods)
        assert got == (size, fo, mo), name
        y = b.download(size + 64)
        assert np.array_equal(y[:size], want) and (y[size:] == CANARY).all(), name
        if len(members) > 1:
            k = kernels_of(ctx)
            assert k["other"][0] == flat_kernels["other"][0] + 1, name
            assert {c: v[0] for c, v in k.items() if c != "other"} == {c: v[0] for c, v in flat_kernels.items() if c != "other"}, name
        s.expect(members, name + ": the pack wrote its members")
    finally:
        s.free()


def test_members_may_repeat_and_the_block_is_kept(pkg, ctx, bufs):
    a, b = bufs
    m = [CA.inputs()[1][:9000], CA.inputs()[6][:5001]]
    members, widths = [m[0], m[1], m[0], m[0][100:4100]], [2, 1, 2, 2]
    lengths = [len(x) for x in members]
    n = sum(lengths)
    cap = pkg.pack_members_bound_auto(lengths, widths)
    ctx.release_memory()
    a.upload(u8(b"".join(members)))
    size, fo, mo = ctx.pack_members_auto_device(a, lengths, widths, b, cap)
    want, kept_flat = b.download(size), ctx.timings().device_bytes
    # the first member three times, once in part: two places of one allocation hold the whole set
    a.upload(u8(b"".join(m)))
    ptrs = [a.ptr, a.ptr + 9000, a.ptr, a.ptr + 100]
    assert ctx.pack_members_ptrs_device(ptrs, lengths, widths, b, cap) == (size, fo, mo)
    assert np.array_equal(b.download(size), want)
    # the gathered set lies in a block that the context keeps, counts, and gives up
    kept = ctx.timings().device_bytes
    assert kept >= kept_flat + n, (kept, kept_flat, n)
    ctx.release_memory()
    a.upload(u8(b"".join(members)))
    ctx.pack_members_auto_device(a, lengths, widths, b, cap)
    assert ctx.timings().device_bytes == kept_flat


def test_pack_refusals(pkg, ctx, bufs):
    a, b = bufs
    L = pkg.lib()
    members, widths = [CA.inputs()[1][:9000], CA.inputs()[6][:5001]], np.array([2, 1], dtype=np.uint32)
    a.upload(u8(b"".join(members)))
    b.upload(np.full(4096, CANARY, dtype=np.uint8))
    ls = np.array([9000, 5001], dtype=np.uint64)
    cap = pkg.pack_members_bound_auto(ls, widths)
    ptrs = lambda *v: np.array(v, dtype=np.uint64)
    got = ctypes.c_uint64(0)

    def call(p=ptrs(a.ptr + 1, a.ptr + 20001), lens=ls, ws=widths, fs=None, count=2, out=b.ptr, room=cap):
        return L.bwts_pack_members_p_device(ctx._h, None if p is None else p.ctypes.data, lens.ctypes.data, ws.ctypes.data, None if fs is None else fs.ctypes.data,
                                            None, count, out, room, ctypes.byref(got), None, None)

    bad_f = np.array([0, 7], dtype=np.uint32)
    for name, rc, want in [
            ("no members", call(count=0), E_ARG), ("a zero length", call(lens=ptrs(9000, 0)), E_ARG), ("a bad width", call(ws=np.array([2, 3], dtype=np.uint32)), E_ARG),
            ("a bad filter", call(fs=bad_f), E_ARG), ("a sum above 2^32", call(lens=ptrs(1 << 32, 1)), E_RANGE), ("an output off its boundary", call(out=b.ptr + 8), E_ARG),
            ("the contiguous call's refusals come first", call(p=None, lens=ptrs(1 << 32, 1)), E_RANGE),
            ("no table", call(p=None), E_ARG), ("a NULL entry", call(p=ptrs(a.ptr, 0)), E_ARG),
            ("a NULL entry before an overlap", call(p=ptrs(0, b.ptr + 100)), E_ARG),
            ("a member inside the output", call(p=ptrs(a.ptr, b.ptr + cap - 1)), E_ARG),
            ("a member across the output's start", call(p=ptrs(b.ptr - 9000 + 1, a.ptr)), E_ARG)]:
        assert rc == want, name
    assert (b.download(4096) == CANARY).all(), "a refused call wrote something"
    # a member that ends where the output begins is beside it
    assert call(p=ptrs(a.ptr + 16384 - 14001, a.ptr + 16384 - 5001), out=a.ptr + 16384, room=cap) == 0


# ---- unpack ----
@pytest.fixture(scope="module")
def golden(ctx):
    """The version-3 golden frame (the model's) on the device, its members, and a slots allocation for up to five destinations"""
    members = C3.golden_set()[0]
    f = u8(C3.golden_frame())
    d = ctx.alloc(f.size + 64)
    d.upload(f)
    yield members, f, d
    d.free()


def unpack_into(ctx, golden, indices, extra=0, every=False):
    """The members named into guarded slots, in reverse address order, each destination `extra` bytes larger than its member"""
    members, f, d = golden
    named = [members[k] for k in indices]
    places, at = [None] * len(named), 64
    for j in reversed(range(len(named))):
        places[j] = (at | 1, len(named[j]))
        at = ((at | 1) + len(named[j]) + extra + 2 * GUARD + 15) // 16 * 16
    s = Slots(ctx, places, at + 64)
    try:
        s.fill()
        ctx.unpack_members_ptrs_device(d, f.size, None if every else indices, s.ptrs(), [len(m) + extra for m in named])
        s.expect(named, "unpack of %s" % (indices,))
    finally:
        s.free()


def test_unpack_into_separate_buffers(ctx, golden):
    unpack_into(ctx, golden, [0, 1, 2, 3], every=True)
    unpack_into(ctx, golden, [0, 1, 2, 3])
    unpack_into(ctx, golden, [3, 1, 3, 0])                  # a subset, with a repeat, in reverse order
    unpack_into(ctx, golden, [2])
    unpack_into(ctx, golden, [0, 1, 2, 3], extra=50, every=True)      # larger destinations: only len bytes are written
    unpack_into(ctx, golden, [1, 1], extra=1)


def test_unpack_refusals_in_order(pkg, ctx, golden):
    members, f, d = golden
    L = pkg.lib()
    lens = [len(m) for m in members]
    places, at = [], 64
    for ln in lens:
        places.append((at, ln))
        at += (ln + 2 * GUARD + 15) // 16 * 16
    s = Slots(ctx, places, at + 64)
    bad = ctx.alloc(f.size)
    try:
        s.fill()
        arr = lambda *v: np.array(v, dtype=np.uint64)
        P, room, idx = arr(*s.ptrs()), arr(*lens), arr(0, 1, 2, 3)

        def call(frame=d.ptr, nbytes=f.size, ix=idx, count=4, p=P, r=room):
            return L.bwts_unpack_members_p_device(ctx._h, frame, nbytes, None if ix is None else ix.ctypes.data, count, None if p is None else p.ctypes.data,
                                                  None if r is None else r.ctypes.data)

        short, null = arr(lens[0], lens[1] - 1, lens[2], lens[3]), arr(P[0], P[1], 0, P[3])
        shared = arr(P[0], P[0] + lens[0] - 1, P[2], P[3])
        for name, rc, want in [
                ("no frame", call(frame=None), E_ARG), ("no bytes", call(nbytes=0), E_ARG), ("a frame off its boundary", call(frame=d.ptr + 8), E_ARG),
                ("a truncated frame", call(nbytes=f.size - 16), E_FORMAT), ("a truncated frame and no table", call(nbytes=f.size - 16, p=None, r=None), E_FORMAT),
                ("no indices, another count", call(ix=None, count=3), E_ARG), ("no destinations asked", call(count=0), E_ARG),
                ("an index past the frame", call(ix=arr(0, 1, 4, 3)), E_RANGE), ("an index past the frame and no table", call(ix=arr(0, 1, 4, 3), p=None), E_RANGE),
                ("no table", call(p=None), E_ARG), ("no rooms", call(r=None), E_ARG), ("a NULL entry", call(p=null), E_ARG),
                ("a NULL entry before a short room", call(p=null, r=short), E_ARG),
                ("a short room", call(r=short), E_SPACE), ("a short room before shared bytes", call(p=shared, r=short), E_SPACE),
                ("no room at all", call(r=arr(0, 0, 0, 0)), E_SPACE),
                ("two destinations share a byte", call(p=shared), E_ARG), ("the same destination twice", call(ix=arr(1, 1), count=2, p=arr(P[1], P[1]), r=arr(lens[1], lens[1])), E_ARG),
                ("a destination inside the frame", call(p=arr(P[0], P[1], d.ptr + f.size - 1, P[3])), E_ARG),
                ("a destination across the frame's start", call(p=arr(P[0], d.ptr - lens[1] + 1, P[2], P[3])), E_ARG)]:
            assert rc == want, name
        s.expect([bytes([CANARY]) * ln for ln in lens], "a refused call wrote something")
        # a sound directory over damaged streams: the checksum's refusal and the coder's, with nothing written anywhere
        at = 19416
        assert f.size == 19472
        for where, code in ((at, E_CHECKSUM), (f.size - 5, E_FORMAT)):
            hurt = f.copy()
            hurt[where] ^= 0x5A
            with pytest.raises(M3.PackError) as e:
                M3.unpack(hurt.tobytes())
            assert e.value.code == code, "the model's refusal of a flipped byte at %d" % where
            bad.upload(hurt)
            assert call(frame=bad.ptr) == code, where
            assert call(frame=bad.ptr, ix=arr(3, 0, 3, 1), r=arr(lens[3], lens[0], lens[3], lens[1]), p=arr(P[3], P[0], P[2], P[1])) == code, where
            s.expect([bytes([CANARY]) * ln for ln in lens], "a call that failed with %d wrote a destination" % code)
        assert call() == 0
        s.expect(members, "unpack after the refusals")
    finally:
        s.free()
        bad.free()


# ---- tensor sets ----
class DevTensor:
    """What pack_tensors asks of a tensor, over bytes of a device allocation"""

    def __init__(self, ptr, nbytes, itemsize):
        self.ptr, self.nbytes, self.itemsize = ptr, nbytes, itemsize

    def data_ptr(self):
        return self.ptr

    def element_size(self):
        return self.itemsize

    def numel(self):
        return self.nbytes // self.itemsize

    def is_contiguous(self):
        return True


def test_tensor_sets_there_and_back(pkg, ctx):
    ma = CA.inputs()
    walk = C3.walk(200000, 4, 77)
    # (bytes, element size): widths 4, 2, 8, 1 and 16 (taken as 1), a 200 000-byte array that is cut, a zero-length one
    data = [(ma[0][:30000], 4), (ma[1][:40002], 2), (b"", 4), (walk, 4), (ma[5][:8 * 1000], 8), (ma[6][:5001], 1), (ma[2][:16 * 100], 16), (ma[4][:30000], 2)]
    sizes = [len(x) for x, _ in data]
    places, at = [], 64
    for b in sizes:
        places.append((at, b))
        at += (b + 2 * GUARD + 15) // 16 * 16
    src, dst = Slots(ctx, places, at + 64), Slots(ctx, places, at + 64)
    try:
        src.fill([x for x, _ in data])
        dst.fill()
        tensors = [DevTensor(p, b, w) for p, b, (_, w) in zip(src.ptrs(), sizes, data)]
        frames = ctx.pack_tensors(tensors, frame_bytes=65536)
        cut = pkg.tensor_frames(sizes, 65536)
        assert len(frames) == len(cut) and len(cut) >= 5 and [k for fr in cut for k, _, _ in fr].count(3) == 4
        widths = [w if w in (1, 2, 4, 8) else 1 for _, w in data]
        for f, fr in zip(frames, cut):
            assert pkg.frame_members(f) == ([b for _, _, b in fr], [widths[k] for k, _, _ in fr])
            # every frame is a member frame like any other
            assert [bytes(m) for m in ctx.unpack_members(f)] == [data[k][0][off:off + b] for k, off, b in fr]
        ctx.unpack_tensors(frames, [DevTensor(p, b, w) for p, b, (_, w) in zip(dst.ptrs(), sizes, data)])
        dst.expect([x for x, _ in data], "unpack_tensors")
        src.expect([x for x, _ in data], "pack_tensors wrote its tensors")
        # explicit values per tensor are carried to all of a tensor's pieces
        frames = ctx.pack_tensors(tensors, filters=[0, 0, 0, 1, 1, 0, 0, 0], methods=[1, 1, 0, 1, 0, 0, 1, 1], frame_bytes=65536)
        for f, fr in zip(frames, cut):
            assert pkg.frame_member_filters(f) == [int(k in (3, 4)) for k, _, _ in fr]
            assert pkg.frame_member_methods(f) == [int(k in (0, 1, 3, 6, 7)) for k, _, _ in fr]
        with pytest.raises(pkg.BwtsError) as e:
            ctx.unpack_tensors(frames, [DevTensor(p, b + (k == 1) - (k == 3), 1) for k, (p, b) in enumerate(zip(dst.ptrs(), sizes))])
        assert e.value.code == E_ARG
    finally:
        src.free()
        dst.free()
