"""GPU suite (-m gpu): the packed radix passes of round 0 (csrc/radix.hip: radix_scatter_packed_kernel in its first, middle and
last form, radix_scatter_lean_last_kernel) after their LDS path changed: no byte table of the slots' digits (a thread takes the
digit from the word it reads in the first write-out and keeps the slot's destination base for the second), and the digit's base
folded into the waves' starts (digit_bases_folded), so that staging an item reads one word.

Every cell is one forward through Context.forward on a fresh context, compared byte for byte with oracle_lib.forward, and header
word 9 of the engine's report ("keys") must name the form round 0 kept its keys in.  The knobs are set the way
tests/test_lean_last_pass.py sets them (BWTS_TEST_KNOBS=1 BWTS_POISON=1, the direct form's gate open, an inherited BWTS_RX_LEAN out
of the way); BWTS_VARLEN=1 BWTS_KEY_BITS=32 / 40 pick keys without and with the high byte (four and five passes, both HI16 forms),
and BWTS_RX_LEAN=0 / unset the classic and the lean last pass.

Sizes.  n = 8191, 8192, 8193, 3 * 8192 + 5 and 65 539 are the sizes the change was asked to be tested at.  The packed passes take a
sort from 65 536 elements on (radix_packed_applicable), so of these only 65 539 reaches the kernels under test: below, round 0 keeps
wide keys, the report says so, and the cells pin that and the bytes.  What the small sizes were chosen for -- a last tile of 8191
elements, none, one element, a seam with five behind it -- is therefore also run at 65 536 + each of them, where word 9 must read
split32 / split40.

Two inputs put the waves' counters at their extremes.  `one_digit`: 0^(n-1) 1 under 1-bit symbols: every key of the first tiles
is zero, so all 1024 elements of a wave hold one digit, one counter takes sixteen steps of 64 and the folded start of every other
digit equals its neighbour's.  `distinct_digits`: any 64 consecutive positions hold 64 different byte values, so in the first pass
no two lanes of a ranking step share a digit: every counter moves by one, and a digit that an item holds has been met by the
wave's earlier items anywhere from never to several times."""
import numpy as np
import pytest

import forward_cases as FC
import key_cases as KC
import oracle_lib as O

from test_lean_last_pass import NOT_TRIED, TILE, run

pytestmark = pytest.mark.gpu

PACKED_FROM = 65536                       # csrc/radix.hip, radix_packed_applicable
ASKED = [8191, 8192, 8193, 3 * 8192 + 5, 65539]
SIZES = ASKED + [PACKED_FROM + n for n in ASKED[:4]]
KEY_BITS = (32, 40)
LEAN = (None, "0")                        # BWTS_RX_LEAN: unset (the lean last pass where the engine picks it), off


def four_letters(n):
    return FC.noise(n, 4, 11)


def geometric200(n):
    """200 letters, letter i about 0.98^i as likely as the first; every letter occurs (code words of up to 12 bits)."""
    x = KC.geometric_text(n, 200, 0.98, 5, base=20)
    x[:200] = np.arange(20, 220, dtype=np.uint8)
    return x


ALPHABETS = {"four": four_letters, "geo200": geometric200}


def keys_word(key_bits, n):
    if n < PACKED_FROM:
        return "wide"
    return "split32" if key_bits <= 32 else "split40"


def check_cells(pkg, x, envs):
    """envs: [(knobs, key symbols or None, key bits expected, keys form expected)]; every cell with the lean switch unset and off."""
    want = O.forward(x)
    for knobs, m, key_bits, keys in envs:
        for lean in LEAN:
            env = dict(knobs, **({} if lean is None else {"BWTS_RX_LEAN": lean}))
            got, _, reps = run(pkg, x, m, env=env)
            rep = reps[-1]
            assert np.array_equal(got, want), (env, np.flatnonzero(got != want)[:8])
            assert rep["cyclic"] and rep["key_bits"] == key_bits and rep["keys"] == keys, (env, rep)
            if lean == "0" or keys != "split40":
                assert rep["lean_word"] == NOT_TRIED, (env, rep)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
def test_sizes(pkg, alphabet, n):
    x = ALPHABETS[alphabet](n)
    assert x.size == n and np.unique(x).size == (4 if alphabet == "four" else 200)
    assert (n % TILE) in (8191, 0, 1, 5, 3) and (n < PACKED_FROM) == (n in ASKED[:4])
    check_cells(pkg, x, [({"BWTS_VARLEN": "1", "BWTS_KEY_BITS": str(kb)}, None, kb, keys_word(kb, n)) for kb in KEY_BITS])


N_EXTREME = PACKED_FROM + TILE + 37


def first_pass_digits(x, bits, m):
    """Digit of the first pass (key bits 0 .. 7) of every position of a one-factor input under fixed-width keys of m symbols."""
    n = x.size
    assert O.lyndon_starts(x).tolist() == [0] and 8 % bits == 0
    p = np.arange(n)
    d = np.zeros(n, dtype=np.int64)
    for j in range(8 // bits):
        d |= x[(p + m - 1 - j) % n].astype(np.int64) << (bits * j)
    return d


def test_one_digit(pkg):
    x = np.zeros(N_EXTREME, dtype=np.uint8)
    x[-1] = 1
    for m in KEY_BITS:
        d = first_pass_digits(x, 1, m)
        assert not d[:N_EXTREME - TILE].any(), "whole tiles of one digit"
    check_cells(pkg, x, [({}, m, m, keys_word(m, x.size)) for m in KEY_BITS])


def test_distinct_digits(pkg):
    n = N_EXTREME
    rng = np.random.default_rng(23)
    perm = rng.permutation(64)
    perm[np.flatnonzero(perm == 0)[0]], perm[0] = perm[0], 0
    r = rng.integers(0, 4, size=n)
    r[::64] = rng.integers(1, 4, size=r[::64].size)              # (the only 0 of the input is its first byte: one Lyndon factor)
    x = (4 * perm[np.arange(n) % 64] + r).astype(np.uint8)
    x[0] = 0
    assert np.unique(x).size > 128
    for m in (4, 5):
        d = first_pass_digits(x, 8, m)
        whole = (n - m) // 64                                    # the 64-lane steps whose keys' last symbols do not wrap
        steps = d[:64 * whole].reshape(whole, 64)
        assert all(np.unique(s).size == 64 for s in steps), "no two lanes of a step share a digit"
        wave = d[:1024].reshape(16, 64)
        firsts = [int((wave[:8] == wave[8 + j // 64, j % 64]).sum()) for j in range(512)]
        assert min(firsts) == 0 and max(firsts) >= 4, "items 8 .. 15 find their digit among items 0 .. 7 from never to several times"
    check_cells(pkg, x, [({}, m, 8 * m, keys_word(8 * m, n)) for m in (4, 5)])
