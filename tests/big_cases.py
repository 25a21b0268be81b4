"""Inputs beyond 2^32 bytes whose move-to-front ranks and entropy-coded stream a few MiB of CPU model output determine, byte for byte.

The input is periodic: one period of P = 2 MiB (eight blocks of the entropy coder; seven of uniform bytes, one of ranks with runs; all
256 byte values occur), repeated q times, and the period's first bytes once more as a tail.  Then
  * move-to-front is periodic from the second period on: every symbol occurs in every period, so the list at a position i >= P is
    fixed by the order of the last occurrences in the P bytes in front of it, and mtf(x)[i + P] == mtf(x)[i] for P <= i < n - P;
  * the coder's stream is an assembly of the model's streams of one period and of the tail: a table depends on its block's bytes
    alone, a payload on its tile's bytes and that table, and P is a whole number of blocks.
A device result of this kind is checked by the CPU model on its first periods, one compare on the device of the result with itself
shifted by a period, and downloaded windows.  tests/test_big_cases.py checks these statements on the CPU at small q."""
import functools

import numpy as np

import ec_model as E
import mtf_model as M

BLOCK = E.K * E.T                        # 256 KiB: the bytes that share one table
P = 8 * BLOCK                            # 2 MiB
TAIL = 12345                             # the last MTF tile, the last EC tile and the last EC block are partial
SEED = 20240
RUNS_BLOCK = 5                           # which block of the period holds ranks with runs (not the first)
N_SINGLE = (1 << 32) + (1 << 29) + TAIL  # positions and stream offsets both cross 2^32
Q_SINGLE = N_SINGLE // P                 # 2304
UPLOAD_PERIODS = 32
# P divides 2^32, so x[i - 2^32] == x[i]: a position that lost its bit 32 on the way to a READ would fetch the right byte.  A second
# period of seven of the eight blocks does not divide it (2^32 = 2340 P7 + 4 blocks): there such a read is four blocks off.
P7 = 7 * BLOCK


def build_period(seed=SEED, blocks=8, block=BLOCK, runs_block=RUNS_BLOCK):
    """blocks x block bytes: uniform bytes, and in block runs_block min(geometric(0.3) - 1, 255), each value 1 to 5 times."""
    assert 0 < runs_block < blocks
    rng = np.random.default_rng(seed)
    per = rng.integers(0, 256, blocks * block, dtype=np.uint8)
    vals = np.minimum(rng.geometric(0.3, block) - 1, 255).astype(np.uint8)
    per[runs_block * block:(runs_block + 1) * block] = np.repeat(vals, rng.integers(1, 6, block))[:block]
    return per


@functools.lru_cache(maxsize=None)
def period():
    per = build_period()
    assert per.size == P and np.unique(per).size == 256
    per.setflags(write=False)
    return per


def periodic(per, n):
    """The first n bytes of per repeated for ever (small n: the CPU tests)."""
    return np.resize(per, n)


# -- the stream of a periodic input, from the model's streams of one period and of the tail ---------------------------------
def stream_parts(stream, n):
    """(tables, directory entries without padding, payloads) of the model's stream of an input of n bytes."""
    s = np.frombuffer(bytes(stream), dtype=np.uint8)
    nt = E.tiles(n)
    nb = E.blocks(nt)
    d0 = 16 + 512 * nb
    return s[16:d0], s[d0:d0 + 4 * nt], s[E.fixed_bytes(n):]


class PeriodicStream:
    """The version-1 stream of per x q + per[:tail], kept as its parts: window(at, size) gives any bytes of it."""

    def __init__(self, per, q, tail):
        per = np.asarray(per, dtype=np.uint8)
        assert per.size % BLOCK == 0 and q >= 1 and 0 <= tail < per.size
        self.q, self.tail, self.n = q, tail, q * per.size + tail
        self.tables_p, self.dir_p, self.pay_p = stream_parts(E.encode(per), per.size)
        empty = np.zeros(0, dtype=np.uint8)
        self.tables_t, self.dir_t, self.pay_t = stream_parts(E.encode(per[:tail]), tail) if tail else (empty, empty, empty)
        self.S = self.pay_p.size                                   # payload bytes of one period
        self.tiles_p = per.size // E.T
        nt = E.tiles(self.n)
        assert nt == q * self.tiles_p + E.tiles(tail)
        header = np.frombuffer(np.array([E.MAGIC, E.PARAMS, self.n & 0xFFFFFFFF, self.n >> 32], dtype="<u4").tobytes(), dtype=np.uint8)
        pad = np.zeros(E.pad16(4 * nt) - 4 * nt, dtype=np.uint8)
        # (piece, times it is repeated), in stream order
        self.pieces = [(header, 1), (self.tables_p, q), (self.tables_t, 1), (self.dir_p, q), (self.dir_t, 1), (pad, 1),
                       (self.pay_p, q), (self.pay_t, 1)]
        self.dir_at = 16 + 512 * E.blocks(nt)
        self.fixed = E.fixed_bytes(self.n)
        assert self.fixed == self.dir_at + E.pad16(4 * nt)
        self.total = self.fixed + q * self.S + self.pay_t.size

    def window(self, at, size):
        assert 0 <= at and size >= 0 and at + size <= self.total
        out = np.empty(size, dtype=np.uint8)
        begin = 0
        for piece, times in self.pieces:
            end = begin + piece.size * times
            lo, hi = max(at, begin), min(at + size, end)
            if lo < hi:
                out[lo - at:hi - at] = piece[(np.arange(lo, hi, dtype=np.int64) - begin) % piece.size]
            begin = end
        return out

    def assemble(self):
        return np.concatenate([np.tile(piece, times) for piece, times in self.pieces])

    def dir_entry(self, t):
        """The directory entry of tile t, and where its payload starts in the stream."""
        sizes_p = self.dir_p.view("<u4").astype(np.int64)
        k, j = divmod(t, self.tiles_p)
        if k == self.q:
            sizes_t = self.dir_t.view("<u4").astype(np.int64)
            return int(sizes_t[j]), self.fixed + self.q * self.S + int(sizes_t[:j].sum())
        return int(sizes_p[j]), self.fixed + k * self.S + int(sizes_p[:j].sum())


def assemble_stream(sp, st, q, n):
    """The stream of an input of n bytes, q periods and a tail, from the model's streams sp of one period and st of the tail alone:
    the header for n; q copies of sp's tables, then st's; q copies of sp's directory entries, then st's, then zeros to 16; q copies of
    sp's payloads, then st's."""
    nt_p, nt = E.tiles(P), E.tiles(n)
    tail = n - q * P
    assert 0 < tail < P and nt == q * nt_p + E.tiles(tail)
    tp, dp, pp = stream_parts(sp, P)
    tt, dt, pt = stream_parts(st, tail)
    parts = [np.array([E.MAGIC, E.PARAMS, n & 0xFFFFFFFF, n >> 32], dtype="<u4").tobytes(), tp.tobytes() * q, tt.tobytes(),
             dp.tobytes() * q, dt.tobytes(), bytes(E.pad16(4 * nt) - 4 * nt), pp.tobytes() * q, pt.tobytes()]
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def single_stream():
    """The expected stream of the single-input tests (N_SINGLE bytes)."""
    return PeriodicStream(period(), Q_SINGLE, TAIL)


def expected_stream_window(at, size):
    """Bytes [at, at + size) of the stream of the N_SINGLE-byte input, without the stream."""
    return single_stream().window(at, size)


@functools.lru_cache(maxsize=None)
def seven_block_case():
    """The same N_SINGLE bytes from the period's first seven blocks: (period, its stream)."""
    per = period()[:P7]
    assert np.unique(per).size == 256 and (1 << 32) % P7 == 4 * BLOCK
    return per, PeriodicStream(per, N_SINGLE // P7, N_SINGLE % P7)


@functools.lru_cache(maxsize=None)
def seven_block_mtf_model():
    """mtf of the first two periods of that input."""
    return np.frombuffer(M.forward_fast(periodic(period()[:P7], 2 * P7).tobytes()), dtype=np.uint8)


def size_ok(size, length):
    """ec_size_ok of ec_plan.h: a payload of a tile of `length` bytes."""
    return size >= 256 and size % 16 == 0 and size <= E.pad16(256 + 2 * length)


# -- move-to-front of a periodic input ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_mtf_model():
    """mtf of the first 2 P + TAIL bytes of the periodic input: all the model output the N_SINGLE-byte case needs."""
    return np.frombuffer(M.forward_fast(periodic(period(), 2 * P + TAIL).tobytes()), dtype=np.uint8)


def mtf_expected(model, period_bytes, at, size):
    """mtf(x)[at : at + size] of a periodic x from the model's output over (at least) its first two periods."""
    i = np.arange(at, at + size, dtype=np.int64)
    return model[np.where(i < period_bytes, i, period_bytes + (i - period_bytes) % period_bytes)]


# -- device plumbing ------------------------------------------------------------------------------------------------------------
def upload_at(pkg, ctx, ptr, at, data):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    ctx._check(pkg.lib().bwts_copy_to_device(ctx._h, ptr + at, a.ctypes.data, a.size))


def download_at(pkg, ctx, ptr, at, size):
    out = np.empty(size, dtype=np.uint8)
    ctx._check(pkg.lib().bwts_copy_to_host(ctx._h, out.ctypes.data, ptr + at, size))
    return out


def upload_periodic(pkg, ctx, ptr, per, n):
    """The first n bytes of per repeated, from one host block of UPLOAD_PERIODS periods."""
    block = np.tile(per, UPLOAD_PERIODS)
    for at in range(0, n, block.size):
        upload_at(pkg, ctx, ptr, at, block[:min(block.size, n - at)])
