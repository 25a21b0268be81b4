"""Move-to-front (include/bwts_mtf.h) and the entropy coder (include/bwts_ec.h) on a device beyond 2^32 bytes: one input of
2^32 + 2^29 + 12345 bytes, whose positions and whose coded stream both cross 2^32; the segment forms at a sum of exactly 2^32; the same
n from a period that does not divide 2^32; and both stages behind the 64-bit transform at 2^32 + 2^28 + 12345.  Every output byte is
covered: the inputs are periodic (tests/big_cases.py),
so the CPU models' output over the first periods, one compare on the device of a result with itself a period further on, and downloaded
windows decide all of it.  Every comparison is exact.

The tests share four device buffers (x: the periodic input, m and r: byte sides, s: the coded side) and each makes what it needs."""
import ctypes

import numpy as np
import pytest

import big_cases as B
import ec_model as E
import mtf_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

E_NOMEM, E_RANGE, E_FORMAT, E_SPACE = -3, -5, -8, -9
P, N, Q = B.P, B.N_SINGLE, B.Q_SINGLE
TWO32 = 1 << 32
GUARD = np.full(64, 0xA5, dtype=np.uint8)


class Big:
    def __init__(self, pkg, ctx, bufs):
        self.pkg, self.ctx = pkg, ctx
        self.x, self.m, self.r, self.s = bufs
        self.per = B.period()
        self.ps = B.single_stream()
        self.m_holds = self.s_holds = None

    def up(self, buf, at, data):
        B.upload_at(self.pkg, self.ctx, buf.ptr, at, data)

    def down(self, buf, at, size):
        return B.download_at(self.pkg, self.ctx, buf.ptr, at, size)

    def x_window(self, at, size):
        return self.per[np.arange(at, at + size, dtype=np.int64) % P]

    def mtf_of_x(self):
        if self.m_holds != "mtf":
            self.m_holds = None
            self.ctx.mtf_forward_device(self.x, N, self.m)
            self.m_holds = "mtf"

    def stream_of_x(self):
        """x coded into s with out_cap exactly the predicted size, a guard behind it."""
        if self.s_holds != "stream":
            self.s_holds = None
            self.up(self.s, self.ps.total, GUARD)
            size = self.ctx.ec_encode_device(self.x, N, self.s, self.ps.total)
            assert size == self.ps.total, (size, self.ps.total)
            assert np.array_equal(self.down(self.s, self.ps.total, 64), GUARD)
            self.s_holds = "stream"


@pytest.fixture(scope="module")
def big(pkg, ctx):
    ps = B.single_stream()
    assert ps.total > TWO32 and ps.total <= E.bound(N)               # from the model, before anything runs on the device
    bufs = []
    try:
        for size in (N, N, N, ps.total + 64):
            bufs.append(ctx.alloc(size))
        g = Big(pkg, ctx, bufs)
        B.upload_periodic(pkg, ctx, g.x.ptr, g.per, N)
        yield g
    finally:
        for d in bufs:
            d.free()


def _differs(y, want):
    return "first difference at %d of %d" % (int(np.flatnonzero(y != want)[0]), y.size) if y.size == want.size else "sizes %d and %d" % (y.size, want.size)


def _same(y, want, what):
    assert np.array_equal(y, want), "%s: %s" % (what, _differs(y, want))


def test_the_compare_sees_beyond_2p32(big):
    """a. What everything below rests on: the upload is periodic, and device_equal notices one byte behind 2^32."""
    ctx, x, m = big.ctx, big.x, big.m
    assert ctx.device_equal(x.ptr + P, x.ptr + 2 * P, N - 2 * P)
    for at, size in ((0, 1 << 17), (TWO32 - (1 << 16), 1 << 17), (N - (1 << 17), 1 << 17), (3 * P - 100, 200)):
        _same(big.down(x, at, size), big.x_window(at, size), "x at %d" % at)
    big.m_holds = None
    B.upload_periodic(big.pkg, ctx, m.ptr, big.per, N)               # the copy
    assert ctx.device_equal(x, m, N)
    at = TWO32 + 777
    byte = big.down(m, at, 1)
    assert byte[0] == big.per[at % P]
    big.up(m, at, byte ^ 0x01)
    assert not ctx.device_equal(x, m, N)
    assert ctx.device_equal(x, m, at) and ctx.device_equal(x.ptr + at + 1, m.ptr + at + 1, N - at - 1)
    assert not ctx.device_equal(x.ptr + P, m.ptr + P, N - P)         # ... nor a start off zero hides it
    big.up(m, at, byte)
    assert ctx.device_equal(x, m, N)


def test_mtf_forward(big):
    """b. mtf_forward_device at n: the model over the first two periods, the shifted compare over [P, n - P), windows by index."""
    model = B.single_mtf_model()
    big.mtf_of_x()
    _same(big.down(big.m, 0, 2 * P), model[:2 * P], "first two periods")
    assert big.ctx.device_equal(big.m.ptr + P, big.m.ptr + 2 * P, N - 2 * P)
    for at in (0, TWO32 - (1 << 16), N - (1 << 17)):
        _same(big.down(big.m, at, 1 << 17), B.mtf_expected(model, P, at, 1 << 17), "ranks at %d" % at)
    assert not np.array_equal(model[:P], model[P:2 * P])              # the first period starts from the identity


def test_mtf_inverse(big):
    """c. mtf_inverse_device of that output is x; and the inverse of x itself (any bytes are ranks), put forward again, is x."""
    ctx, x, m, r = big.ctx, big.x, big.m, big.r
    big.mtf_of_x()
    ctx.mtf_inverse_device(m, N, r)
    assert ctx.device_equal(r, x, N)
    big.m_holds = None
    ctx.mtf_inverse_device(x, N, r)
    want = np.frombuffer(M.inverse_fast(big.per[:1 << 20].tobytes()), dtype=np.uint8)
    _same(big.down(r, 0, 1 << 20), want, "inverse of x, first MiB")
    ctx.mtf_forward_device(r, N, m)
    assert ctx.device_equal(m, x, N)


def test_ec_encode(big):
    """d. ec_encode_device at n into exactly the predicted size: size, header, all tables, the whole directory, every payload."""
    ctx, s, ps = big.ctx, big.s, big.ps
    big.stream_of_x()                                                 # (asserts the size and the guard)
    head = big.down(s, 0, 16).view("<u4").tolist()
    assert head == [E.MAGIC, E.PARAMS, N & 0xFFFFFFFF, N >> 32] and head[3] == 1
    _same(big.down(s, 0, ps.fixed), ps.window(0, ps.fixed), "header, tables and directory")
    pay = s.ptr + ps.fixed
    assert ctx.device_equal(pay, pay + ps.S, (Q - 1) * ps.S)
    _same(big.down(s, ps.fixed, 2 * ps.S), ps.window(ps.fixed, 2 * ps.S), "payloads of the first two periods")
    at = TWO32 - (1 << 17)
    _same(big.down(s, at, 1 << 18), ps.window(at, 1 << 18), "payloads across stream offset 2^32")
    t = TWO32 // E.T                                                  # the block that holds input position 2^32: 16 tiles from t on
    assert t % E.K == 0 and t // (P // E.T) < Q
    at = ps.dir_entry(t)[1]
    size = ps.dir_entry(t + E.K)[1] - at
    assert size > E.K * 256
    _same(big.down(s, at, size), ps.window(at, size), "payloads of the block at input position 2^32")
    at = ps.total - ps.pay_t.size - ps.S
    _same(big.down(s, at, ps.total - at), ps.window(at, ps.total - at), "payloads of the last period and the tail")
    # 16 bytes less room: refused, and nothing written
    first = big.down(s, 0, 4096)
    mark = np.full(4096, 0xA5, dtype=np.uint8)
    big.s_holds = None
    big.up(s, 0, mark)
    got = ctypes.c_uint64(77)
    rc = big.pkg.lib().bwts_ec_encode_device(ctx._h, big.x.ptr, N, s.ptr, ps.total - 16, ctypes.byref(got))
    assert rc == E_SPACE and got.value == 77
    _same(big.down(s, 0, 4096), mark, "stream start after E_SPACE")
    _same(big.down(s, ps.total, 64), GUARD, "guard after E_SPACE")
    big.up(s, 0, first)
    big.s_holds = "stream"


def test_ec_decode(big):
    """e. ec_decode_device of that stream is x; a directory whose sizes still add up but cut a payload beyond stream offset 2^32
    wrongly is refused by decoding."""
    ctx, s, r, ps = big.ctx, big.s, big.r, big.ps
    big.stream_of_x()
    assert ctx.ec_decode_device(s, ps.total, r, N) == N
    assert ctx.device_equal(r, big.x, N)
    t = 2200 * (P // E.T) + 3
    (s0, at0), (s1, _) = ps.dir_entry(t), ps.dir_entry(t + 1)
    assert at0 > TWO32 and B.size_ok(s0 + 16, E.T) and B.size_ok(s1 - 16, E.T)      # ec_plan.h's rule accepts both
    where = ps.dir_at + 4 * t
    good = big.down(s, where, 8)
    assert good.view("<u4").tolist() == [s0, s1]
    big.s_holds = None
    big.up(s, where, np.array([s0 + 16, s1 - 16], dtype="<u4").view(np.uint8))
    got = ctypes.c_uint64(0)
    rc = big.pkg.lib().bwts_ec_decode_device(ctx._h, s.ptr, ps.total, r.ptr, N, ctypes.byref(got))
    assert rc == E_FORMAT, rc
    big.up(s, where, good)
    big.s_holds = "stream"
    big.up(r, TWO32 - 4096, np.zeros(8192, dtype=np.uint8))
    assert ctx.ec_decode_device(s, ps.total, r, N) == N
    assert ctx.device_equal(r, big.x, N)


def test_segment_forms_at_a_sum_of_2p32(big):
    """f. 1024 pairs of segments of P - 3 and P + 3 bytes of x: two contents, every second segment off a 16-byte boundary."""
    pkg, ctx, x, m, r, s = big.pkg, big.ctx, big.x, big.m, big.r, big.s
    L = pkg.lib()
    ls = np.tile(np.array([P - 3, P + 3], dtype=np.uint64), 1024)
    assert int(ls.sum()) == TWO32
    a, b = big.per[:P - 3], np.concatenate((big.per[P - 3:], big.per))
    _same(big.down(x, 0, 2 * P), np.concatenate((a, b)), "the first pair")
    over = ls.copy()
    over[-1] += 1                                                     # a sum of 2^32 + 1
    # move-to-front
    big.m_holds = None
    ctx.mtf_forward_segments_device(x, ls, m)
    want = np.frombuffer(M.forward_fast(a.tobytes()) + M.forward_fast(b.tobytes()), dtype=np.uint8)
    _same(big.down(m, 0, 2 * P), want, "ranks of the first pair")
    assert ctx.device_equal(m, m.ptr + 2 * P, TWO32 - 2 * P)
    ctx.mtf_inverse_segments_device(m, ls, r)
    assert ctx.device_equal(r, x, TWO32)
    assert L.bwts_mtf_forward_segments_device(ctx._h, x.ptr, over.ctypes.data, over.size, r.ptr) == E_RANGE
    assert ctx.device_equal(r, x, TWO32)
    # the coder
    sa, sb = E.encode(a), E.encode(b)
    pair = len(sa) + len(sb)
    total = 1024 * pair
    assert total + 64 <= s.nbytes
    big.s_holds = None
    big.up(s, total, GUARD)
    sizes = ctx.ec_encode_segments_device(x, ls, s, total)            # exactly the room it needs
    assert np.array_equal(sizes, np.tile(np.array([len(sa), len(sb)], dtype=np.uint64), 1024))
    out = np.zeros(ls.size, dtype=np.uint64)
    rc = L.bwts_ec_encode_segments_device(ctx._h, x.ptr, over.ctypes.data, over.size, s.ptr, total, out.ctypes.data)
    assert rc == E_RANGE and not out.any()
    _same(big.down(s, total, 64), GUARD, "guard behind the streams")
    _same(big.down(s, 0, pair), np.frombuffer(sa + sb, dtype=np.uint8), "streams of the first pair")
    assert ctx.device_equal(s, s.ptr + pair, total - pair)
    big.up(r, 0, np.zeros(1 << 20, dtype=np.uint8))
    ctx.ec_decode_segments_device(s, sizes, ls, r)
    assert ctx.device_equal(r, x, TWO32)


def test_a_period_that_does_not_divide_2p32(big):
    """h. b to e in short on the same n bytes made from seven of the period's eight blocks.  P divides 2^32, so above x[i - 2^32] == x[i]
    and a position that lost bit 32 on its way to a read would still fetch the right byte; here such a read is four blocks off."""
    pkg, ctx, x, m, r, s = big.pkg, big.ctx, big.x, big.m, big.r, big.s
    per, ps = B.seven_block_case()
    model = B.seven_block_mtf_model()
    P7 = B.P7
    assert ps.n == N and TWO32 < ps.total <= s.nbytes - 64

    def window(at, size):
        return per[np.arange(at, at + size, dtype=np.int64) % P7]

    assert (window(TWO32, B.BLOCK) != window(0, B.BLOCK)).mean() > 0.9
    big.m_holds = big.s_holds = None
    B.upload_periodic(pkg, ctx, m.ptr, per, N)                        # the input: m
    _same(big.down(m, TWO32 - (1 << 16), 1 << 17), window(TWO32 - (1 << 16), 1 << 17), "input across 2^32")
    # move-to-front, and back into x's buffer, which gets its own bytes again afterwards
    ctx.mtf_forward_device(m, N, r)
    _same(big.down(r, 0, 2 * P7), model, "first two periods")
    assert ctx.device_equal(r.ptr + P7, r.ptr + 2 * P7, N - 2 * P7)
    for at in (TWO32 - (1 << 16), N - (1 << 17)):
        _same(big.down(r, at, 1 << 17), B.mtf_expected(model, P7, at, 1 << 17), "ranks at %d" % at)
    try:
        ctx.mtf_inverse_device(r, N, x)
        assert ctx.device_equal(x, m, N)
    finally:
        B.upload_periodic(pkg, ctx, x.ptr, big.per, N)
    # the coder, into exactly the predicted size
    big.up(s, ps.total, GUARD)
    assert ctx.ec_encode_device(m, N, s, ps.total) == ps.total
    _same(big.down(s, ps.total, 64), GUARD, "guard")
    _same(big.down(s, 0, ps.fixed), ps.window(0, ps.fixed), "header, tables and directory")
    pay = s.ptr + ps.fixed
    assert ctx.device_equal(pay, pay + ps.S, (ps.q - 1) * ps.S)
    t = TWO32 // E.T
    at = ps.dir_entry(t)[1]
    last = ps.total - ps.pay_t.size - ps.S
    for lo, size, what in ((ps.fixed, 2 * ps.S, "the first two periods"), (TWO32 - (1 << 17), 1 << 18, "across stream offset 2^32"),
                           (at, ps.dir_entry(t + E.K)[1] - at, "the block at input position 2^32"), (last, ps.total - last, "the last period and the tail")):
        _same(big.down(s, lo, size), ps.window(lo, size), "payloads of " + what)
    assert ctx.ec_decode_device(s, ps.total, r, N) == N
    assert ctx.device_equal(r, m, N)


def _transform(pkg, call, *args):
    try:
        call(*args)
    except pkg.BwtsError as e:
        if e.code == E_NOMEM:
            pytest.skip("not enough free device memory for the transform at 2^32 + 2^28")
        raise


def test_pipeline_behind_the_wide_transform(big):
    """g. forward -> mtf -> encode -> decode -> mtf inverse -> inverse at 2^32 + 2^28 + 12345 bytes of dna: here the two stages take
    their working memory from an arena the 64-bit transform paths have just used.  The way back equals the way out at every step;
    three blocks of ranks and stream are checked against the models."""
    pkg, ctx = big.pkg, big.ctx
    n, seed = TWO32 + (1 << 28) + 12345, 5
    bw, mt, s = big.m, big.r, big.s
    cap = s.nbytes // 16 * 16
    extra = []
    try:
        for _ in range(2):
            extra.append(ctx.alloc(n))
        x, w = extra
        ctx.generate("dna", seed, n, x)
        big.m_holds = big.s_holds = None
        _transform(pkg, ctx.forward_device, x, n, bw)
        ctx.mtf_forward_device(bw, n, mt)                             # (BWTS_E_NOMEM from these is a failure)
        size = ctx.ec_encode_device(mt, n, s, cap)
        assert size % 16 == 0 and E.fixed_bytes(n) + 256 * E.tiles(n) <= size <= E.bound(n)
        # three blocks against the models: the one that holds input position 2^32, the first and the last (partial)
        nt = E.tiles(n)
        nb = E.blocks(nt)
        dir_at = 16 + 512 * nb
        head = big.down(s, 0, 16).view("<u4").tolist()
        assert head == [E.MAGIC, E.PARAMS, n & 0xFFFFFFFF, 1]
        entries = big.down(s, dir_at, 4 * nt)
        offs = E.fixed_bytes(n) + np.concatenate(([0], np.cumsum(entries.view("<u4").astype(np.int64))))
        assert int(offs[-1]) == size
        alphabet = np.unique(O.generate("dna", 1 << 16, seed))
        for blk in (TWO32 // B.BLOCK, 0, nb - 1):
            lo = blk * B.BLOCK
            hi = min(n, lo + B.BLOCK)
            assert blk < nb and (blk != nb - 1 or hi - lo == 12345)
            ranks = big.down(mt, lo, hi - lo)
            tab, ent, pay = B.stream_parts(E.encode(ranks), hi - lo)
            t0 = blk * E.K
            _same(big.down(s, 16 + 512 * blk, 512), tab, "table of block %d" % blk)
            _same(entries[4 * t0:4 * t0 + ent.size], ent, "directory entries of block %d" % blk)
            _same(big.down(s, int(offs[t0]), pay.size), pay, "payloads of block %d" % blk)
            # 64 KiB of ranks against the model run over the transform's output with a 64 KiB lead-in that holds every symbol
            at = lo if blk != nb - 1 else n - (1 << 16)
            lead = min(at, 1 << 16)
            src = big.down(bw, at - lead, lead + (1 << 16))
            assert lead == 0 or np.array_equal(np.unique(src[:lead]), alphabet)
            want = np.frombuffer(M.forward_fast(src.tobytes()), dtype=np.uint8)[lead:]
            _same(big.down(mt, at, 1 << 16), want, "ranks at %d" % at)
        # the way back
        assert ctx.ec_decode_device(s, size, w, n) == n
        assert ctx.device_equal(w, mt, n)
        ctx.mtf_inverse_device(w, n, mt)
        assert ctx.device_equal(mt, bw, n)
        _transform(pkg, ctx.inverse_device, mt, n, w)
        assert ctx.device_equal(w, x, n)
    finally:
        for d in extra:
            d.free()
