"""What tests/big_cases.py states, checked on the CPU at small sizes: the stream of a periodic input is the assembly of the model's
streams of one period and of the tail, any window of it comes out without the whole, move-to-front is periodic from the second
period on, and the sizes of the real case (tests/test_beyond_2p32_gpu.py) are what that suite needs."""
import numpy as np
import pytest

import big_cases as B
import ec_model as E
import mtf_model as M


@pytest.fixture(scope="module")
def small():
    """q = 3 periods and the tail: the input, the model's stream of the whole, and the assembly's parts."""
    per = B.period()
    q = 3
    n = q * B.P + B.TAIL
    x = B.periodic(per, n)
    assert np.array_equal(x[q * B.P:], per[:B.TAIL]) and np.array_equal(x[2 * B.P:3 * B.P], per)
    return per, q, n, E.encode(x), B.PeriodicStream(per, q, B.TAIL)


def test_period_is_as_stated():
    per = B.period()
    assert per.size == B.P == 8 * E.K * E.T and np.unique(per).size == 256
    blocks = per.reshape(8, B.BLOCK)
    for b in range(8):
        zero_ranks = int((blocks[b][1:] == blocks[b][:-1]).sum())
        if b == B.RUNS_BLOCK:
            assert zero_ranks > B.BLOCK // 2 and int(np.median(blocks[b])) <= 2        # runs of small values
        else:
            assert zero_ranks < B.BLOCK // 64 and np.unique(blocks[b]).size == 256      # uniform bytes
    assert np.array_equal(B.build_period(), per)                                        # a fixed seed


def test_assembly_equals_the_model_on_the_whole(small):
    per, q, n, whole, ps = small
    sp, st = E.encode(per), E.encode(per[:B.TAIL])
    assert B.assemble_stream(sp, st, q, n) == whole
    assert ps.total == len(whole) and ps.n == n
    assert ps.assemble().tobytes() == whole
    assert ps.S % 16 == 0 and ps.fixed == E.fixed_bytes(n)


def test_windows_agree_with_slices_of_the_assembly(small):
    per, q, n, whole, ps = small
    w = np.frombuffer(whole, dtype=np.uint8)
    tables_end = 16 + 512 * 8 * q                 # where the tail's table starts
    borders = {"header/tables": 16, "period tables/tail table": tables_end, "tables/directory": ps.dir_at,
               "period entries/tail entry": ps.dir_at + 512 * q, "directory/payload": ps.fixed,
               "period/period": ps.fixed + ps.S, "second period/third": ps.fixed + 2 * ps.S,
               "last period/tail": ps.fixed + q * ps.S}
    assert ps.dir_at == tables_end + 512
    for name, at in borders.items():
        for lo, size in ((at - 1, 2), (max(at - 100, 0), 333), (at - 7, 7), (at, 9)):
            assert np.array_equal(ps.window(lo, size), w[lo:lo + size]), (name, lo, size)
    assert np.array_equal(ps.window(0, ps.total), w)
    assert np.array_equal(ps.window(ps.total - 5, 5), w[-5:]) and ps.window(77, 0).size == 0
    assert np.array_equal(ps.window(ps.fixed - 40, 2 * ps.S + 99), w[ps.fixed - 40:ps.fixed + 2 * ps.S + 59])      # across two borders
    rng = np.random.default_rng(3)
    for lo in rng.integers(0, ps.total - 5000, 20).tolist():
        assert np.array_equal(ps.window(lo, 5000), w[lo:lo + 5000]), lo
    # a directory entry and its payload's place, for tiles of the first, a middle and the last period and the tail
    sizes = w[ps.dir_at:ps.dir_at + 4 * E.tiles(n)].view("<u4").astype(np.int64)
    offs = ps.fixed + np.concatenate(([0], np.cumsum(sizes)))
    for t in (0, 1, 127, 128, 200, 383, 384):
        assert ps.dir_entry(t) == (int(sizes[t]), int(offs[t])), t


def test_mtf_is_periodic_from_the_second_period_on():
    """Against the definition, on a short period of the same build (8 x 1 KiB)."""
    per = B.build_period(seed=5, block=1024)
    p = per.size
    assert np.unique(per).size == 256
    n = 3 * p + 777
    x = B.periodic(per, n)
    y = np.frombuffer(M.forward(x.tobytes()), dtype=np.uint8)
    assert np.array_equal(y[p:n - p], y[2 * p:])                      # mtf(x)[i + P] == mtf(x)[i] for P <= i < n - P
    assert not np.array_equal(y[:p], y[p:2 * p])                      # the first period starts from the identity
    model = np.frombuffer(M.forward(x[:2 * p].tobytes()), dtype=np.uint8)
    assert np.array_equal(B.mtf_expected(model, p, 0, n), y)
    assert np.array_equal(B.mtf_expected(model, p, 2 * p - 5, p + 9), y[2 * p - 5:3 * p + 4])
    assert M.forward_fast(x.tobytes()) == y.tobytes()


def test_the_real_case_crosses_2p32_both_ways():
    ps = B.single_stream()
    n = B.N_SINGLE
    assert n == (1 << 32) + (1 << 29) + 12345 == B.Q_SINGLE * B.P + B.TAIL and B.Q_SINGLE == 2304
    assert ps.n == n and ps.q == B.Q_SINGLE
    assert ps.total > 1 << 32
    assert ps.total <= E.bound(n) and ps.total % 16 == 0
    assert ps.fixed == E.fixed_bytes(n) < 16 << 20
    # windows of the real stream: the header names n with a high word, the directory ends with the tail's entry and zeros
    head = ps.window(0, 16).view("<u4")
    assert head.tolist() == [E.MAGIC, E.PARAMS, n & 0xFFFFFFFF, 1]
    nt = E.tiles(n)
    assert nt == 128 * B.Q_SINGLE + 1 and ps.fixed - (ps.dir_at + 4 * nt) == 12
    assert not ps.window(ps.dir_at + 4 * nt, 12).any()
    assert np.array_equal(ps.window(ps.fixed + 2000 * ps.S - 16, 48), np.concatenate((ps.pay_p[-16:], ps.pay_p[:32])))
    assert np.array_equal(ps.window(ps.total - ps.pay_t.size - 16, ps.pay_t.size + 16), np.concatenate((ps.pay_p[-16:], ps.pay_t)))
    # the tile the malformed case of the GPU suite moves: both sizes stay valid, and its payload lies beyond 2^32
    t = 2200 * 128 + 3
    (s0, at0), (s1, _) = ps.dir_entry(t), ps.dir_entry(t + 1)
    assert at0 > 1 << 32 and B.size_ok(s0 + 16, E.T) and B.size_ok(s1 - 16, E.T)
    assert B.size_ok(256, 1) and not B.size_ok(240, E.T) and not B.size_ok(264, E.T) and not B.size_ok(E.pad16(256 + 2 * E.T) + 16, E.T)


def test_the_seven_block_case():
    """The second input of the GPU suite: its period does not divide 2^32, its tail is more than a block, and its stream crosses 2^32 too.
    The assembly with such a tail, against the model on the whole at q = 2."""
    per, ps = B.seven_block_case()
    assert per.size == B.P7 and ps.n == B.N_SINGLE and ps.tail > B.BLOCK and ps.tail % E.T
    assert ps.total > 1 << 32 and ps.total <= E.bound(B.N_SINGLE)
    assert not np.array_equal(per[:B.BLOCK], per[4 * B.BLOCK:5 * B.BLOCK])
    n = 2 * B.P7 + ps.tail
    small = B.PeriodicStream(per, 2, ps.tail)
    assert small.assemble().tobytes() == E.encode(B.periodic(per, n))
    for t in (0, 111, 112, 223, 224, 230, E.tiles(n) - 1):
        sizes = small.assemble()[small.dir_at:small.dir_at + 4 * E.tiles(n)].view("<u4").astype(np.int64)
        assert small.dir_entry(t) == (int(sizes[t]), small.fixed + int(sizes[:t].sum())), t
