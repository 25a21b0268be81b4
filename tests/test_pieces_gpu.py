"""GPU suite of copy_pieces_kernel alone (csrc/pieces.hip), through bwts_debug_copy_pieces, against numpy slicing: every pairing of
source and destination misalignment, lengths around the tile, many tiny pieces, pieces at both ends of a source allocated at exactly
its size, any order, and the refusals.  The destination is filled with a canary first: every byte no piece covers must stay."""
import numpy as np
import pytest

import pack_range_model as R

pytestmark = pytest.mark.gpu

E_ARG = -1
T = R.T
CANARY = 0xC7


def run_pieces(ctx, src, pieces, dst_bytes, src_skip=0):
    """The pieces of src[src_skip:] (offsets count from there) into a canary-filled destination of dst_bytes; the result must be what
    numpy slicing makes, canaries included.  The source buffer is allocated at exactly src.size bytes."""
    want = np.full(dst_bytes, CANARY, dtype=np.uint8)
    covered = np.zeros(dst_bytes, dtype=bool)
    for s, d, b in pieces:
        assert b >= 1 and s + b <= src.size - src_skip and d >= 32 and d + b + 32 <= dst_bytes
        assert not covered[d - 32:d + b + 32].any(), "a test's pieces keep 32 canary bytes on both sides"
        want[d:d + b] = src[src_skip + s:src_skip + s + b]
        covered[d:d + b] = True
    a, c = ctx.alloc(src.size), ctx.alloc(dst_bytes)
    try:
        a.upload(src)
        c.upload(np.full(dst_bytes, CANARY, dtype=np.uint8))
        ctx.debug_copy_pieces(a.ptr + src_skip, src.size - src_skip, pieces, c, dst_bytes)
        got = c.download(dst_bytes)
    finally:
        a.free()
        c.free()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first wrong byte at %d of %d (%s)" % (bad[0], dst_bytes, "inside a piece" if covered[bad[0]] else "a canary")
    return got


def source(n, seed):
    x = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    x[x == CANARY] = 0      # a copied byte never looks like a canary
    return x


def test_every_misalignment_pair_at_short_lengths(ctx):
    """16 x 16 misalignments x six lengths below three stores: 1536 pieces in one call, every one in a slot of its own."""
    lengths = [1, 15, 16, 17, 31, 33]
    pieces, slot = [], 0
    for sm in range(16):
        for dm in range(16):
            for ln in lengths:
                pieces.append((128 * slot + 16 + sm, 128 * slot + 32 + dm, ln))
                slot += 1
    run_pieces(ctx, source(128 * slot, 1), pieces, 128 * slot)


def test_lengths_around_the_tile(ctx):
    pieces, s, d = [], 0, 64
    for sm, dm in ((1, 0), (0, 1), (5, 11), (0, 0)):
        for ln in (T - 1, T, T + 1, 2 * T + 1):
            pieces.append((s + sm, d + dm, ln))
            s += (ln + 16 + 15) // 16 * 16
            d += (ln + 80 + 15) // 16 * 16
    run_pieces(ctx, source(s + 16, 2), pieces, d + 64)


def test_first_tiles_that_end_at_a_line_of_the_destination(ctx):
    """A piece's first tile is shorter by its destination's offset in a 256-byte line: lengths around that first tile and around the
    second one, at offsets 1, 129 and 255, the source at 0 and at 3 off a 16-byte boundary."""
    pieces, s, d = [], 0, 256
    for lead in (1, 129, 255):
        for ln in (T - lead - 1, T - lead, T - lead + 1, 2 * T - lead, 2 * T - lead + 1, 3 * T):
            for sm in (0, 3):
                pieces.append((s + sm, d + lead, ln))
                s += (ln + 16 + 15) // 16 * 16
                d += (ln + lead + 64 + 255) // 256 * 256
    run_pieces(ctx, source(s + 16, 6), pieces, d + 256)


def test_a_thousand_one_byte_pieces(ctx):
    pieces = [(7 * i, 32 + 33 * i, 1) for i in range(1000)]
    run_pieces(ctx, source(7 * 1000, 3), pieces, 33 * 1000 + 64)


@pytest.mark.parametrize("skip", [0, 3])
def test_both_ends_of_the_source(ctx, skip):
    """One piece from source byte 0 and one that ends at the source's last byte, of a source allocated at exactly its size (no
    multiple of 16) and, with skip, beginning off a 16-byte boundary: the aligned 16-byte pieces around both ends are not the source's."""
    n = 5003 + skip
    m = n - skip
    for first, last in ((1, 1), (17, 40), (100, 2 * 16 + 5), (m // 2, m - m // 2)):
        for dm in (0, 9):
            pieces = [(0, 32 + dm, first), (m - last, 32 + dm + first + 70, last)]
            run_pieces(ctx, source(n, 4 + first), pieces, m + 256, src_skip=skip)


def test_the_whole_source_as_one_piece(ctx):
    for n in (1, 16, T, 3 * T + 5):
        run_pieces(ctx, source(n, n), [(0, 37, n)], n + 128)


def test_pieces_in_any_order(ctx):
    """Destinations descending while the sources ascend, then shuffled; overlapping and repeated sources are fine."""
    k = 40
    lens = [1 + (37 * i) % 300 for i in range(k)]
    dst, at = [], 48
    for ln in lens:
        dst.append(at)
        at += ln + 40
    src = source(4096, 9)
    pieces = [(13 * i, dst[k - 1 - i], lens[k - 1 - i]) for i in range(k)]
    run_pieces(ctx, src, pieces, at + 64)
    order = np.random.default_rng(5).permutation(k)
    run_pieces(ctx, src, [(100, dst[j], lens[j]) for j in order], at + 64)


def test_refusals(pkg, ctx):
    src = source(4096, 11)
    a, c = ctx.alloc(4096), ctx.alloc(4096)
    try:
        a.upload(src)
        c.upload(np.full(4096, CANARY, dtype=np.uint8))
        bad = {"past the source": [(4000, 0, 97)], "past the destination": [(0, 4000, 97)], "source offset wraps": [((1 << 64) - 8, 0, 16)],
               "destination offset wraps": [(0, (1 << 64) - 8, 16)], "bytes wrap": [(8, 8, (1 << 64) - 4)], "no bytes": [(0, 0, 0)],
               "overlapping destinations": [(0, 100, 50), (500, 149, 10)], "the same destination twice": [(0, 100, 50), (0, 100, 50)],
               "one inside another": [(0, 100, 50), (9, 120, 1)], "a good piece before a bad one": [(0, 0, 16), (4090, 64, 7)]}
        for name, pieces in bad.items():
            with pytest.raises(pkg.BwtsError) as e:
                ctx.debug_copy_pieces(a, 4096, pieces, c, 4096)
            assert e.value.code == E_ARG, name
        with pytest.raises(pkg.BwtsError):
            ctx.debug_copy_pieces(a, 4096, [], c, 4096)
        assert (c.download(4096) == CANARY).all(), "a refused call wrote something"
        # touching is not overlapping, and the buffers' last bytes may be used
        ctx.debug_copy_pieces(a, 4096, [(4095, 4095, 1), (0, 100, 50), (7, 150, 10)], c, 4096)
        got = c.download(4096)
        assert got[4095] == src[4095] and np.array_equal(got[100:150], src[:50]) and np.array_equal(got[150:160], src[7:17])
    finally:
        a.free()
        c.free()
