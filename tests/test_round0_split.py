"""Round 0 of the forward transform on the packed radix path: the key builder counts the first pass's digits (the pass then has no
histogram sweep of its own), the cyclic patches move those counts, and the last pass leaves the sorted keys split (low words +
one byte of key bits 32..39) for the group flags, the key directory and the rank searches.  Every case is compared with the CPU
oracle, byte for byte, on inputs placed at the edges of that work: sizes around the radix tile (8192 positions) and the key
builder's tile (2048), many Lyndon factors (patches in every radix tile), keys of <= 32 and of 33..40 bits, the general Lyndon
path, few ties (rank searches in the split keys) and many ties (the dense rank array)."""
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def _check(ctx, x):
    y = ctx.forward(x)
    t = ctx.timings()                   # (the forward's: the inverse below reports its own)
    assert np.array_equal(y, O.forward(x))
    assert np.array_equal(ctx.inverse(y), x)
    return t


def _descending_lyndon_words(n, seed, first=1, lo=2, hi=256, lmin=3, lmax=40):
    """Words whose first byte is smaller than all their other bytes (so each is a Lyndon word), in non-increasing order: the
    input's Lyndon factors are exactly these words."""
    rng = np.random.default_rng(seed)
    words, total = [], 0
    while total < n:
        L = int(rng.integers(lmin, lmax + 1))
        w = bytes([first]) + bytes(rng.integers(lo, hi, size=L - 1, dtype=np.uint8))
        words.append(w)
        total += L
    words.sort(reverse=True)
    return np.frombuffer(b"".join(words)[:n], dtype=np.uint8).copy()


# sizes around tile edges: 1 and the radix tile, then sizes that take the packed passes (>= 65536), whole and partial tiles
@pytest.mark.parametrize("n", [1, 8191, 8192, 8193, 65536, 65537, 8192 * 9 + 1, 8192 * 12 + 2047, 100003, (1 << 20) + 777])
@pytest.mark.parametrize("kind", ["uniform256", "zipf", "dna", "text"])
def test_sizes_at_tile_edges(ctx, kind, n):
    _check(ctx, O.generate(kind, n, n % 97 + 5))


@pytest.mark.parametrize("sigma", [2, 3, 4, 16, 256])
def test_alphabet_sizes(ctx, sigma):
    rng = np.random.default_rng(sigma)
    _check(ctx, rng.integers(0, sigma, size=300001, dtype=np.uint8))


@pytest.mark.parametrize("kind,symbols,bits", [("uniform256", 4, 32), ("uniform256", 5, 40), ("dna", 16, 32), ("dna", 19, 38)])
def test_key_widths(pkg, kind, symbols, bits):
    """Keys of exactly 32 bits (split keys without a high byte) and of 33..40 bits (with one), fixed-width codes forced by the
    symbol-count knob, on sizes that end inside a radix tile."""
    saved = {k: os.environ.get(k) for k in ("BWTS_TEST_KNOBS", "BWTS_KEY_SYMBOLS")}
    os.environ.update(BWTS_TEST_KNOBS="1", BWTS_KEY_SYMBOLS=str(symbols))
    try:
        with pkg.Context(0) as c:
            for n in (65536 + 3, 8192 * 40 + 4097):
                t = _check(c, O.generate(kind, n, symbols))
                assert t.key_bits == bits
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("n,lmax", [(200000, 12), (1 << 20, 40), (3 * 8192 + 5, 3)])
def test_many_factors_patches_cross_tiles(ctx, n, lmax):
    """Tens of thousands of short Lyndon factors: every radix tile holds many factor ends whose keys the patches rewrite, some
    right at the tile boundaries."""
    x = _descending_lyndon_words(n, n, lmax=lmax)
    t = _check(ctx, x)
    assert t.factors > 1000


def test_general_lyndon_path(ctx):
    """More than 65536 factor candidates: the fast factor search gives up, the general path builds the keys again, and the first
    radix pass runs its own histogram sweep."""
    x = _descending_lyndon_words(4 << 20, 3, lmax=20)
    t = _check(ctx, x)
    assert t.factors > 65536         # (every factor start is a candidate)


def test_few_ties_rank_searches(ctx):
    """Random bytes: few positions stay tied after round 0, and the later rounds rank the rest by searches in the sorted keys."""
    x = O.generate("uniform256", 3 << 20, 21)
    t = _check(ctx, x)
    assert t.active_after_round0 < x.size // 32


@pytest.mark.parametrize("period", [b"abcab", b"the quick brown fox "])
def test_many_ties_dense_ranks(ctx, period):
    """A periodic input of 2^22 and more positions: most positions stay tied after round 0 (the dense rank array, built in
    the sorted keys' buffer)."""
    n = (1 << 22) + 4099
    x = np.frombuffer((period * (n // len(period) + 1))[:n - 1] + b"a", dtype=np.uint8).copy()
    t = _check(ctx, x)
    assert t.active_after_round0 > n // 32
