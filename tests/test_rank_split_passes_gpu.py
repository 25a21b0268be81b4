"""GPU suite (-m gpu): the packed radix passes of round 0 (csrc/radix.hip: radix_scatter_packed_kernel first, middle and last,
radix_scatter_lean_last_kernel) with their ranking split between LDS atomics and ballots (rank_split): some of a thread's sixteen
items take one returning LDS add on the wave's u32 counter, the rest the ballot step, on the same counters, which sit in the front
of the stage area until the first staging trip.

The cells are those of tests/test_packed_pass_lds_gpu.py (check_cells: one forward through Context.forward on a fresh context per
cell, BWTS_VARLEN=1, BWTS_KEY_BITS = 32 and 40, BWTS_RX_LEAN unset and 0, bytes equal to oracle_lib.forward, header word 9 split32 /
split40).

Sizes.  65 536 + {0, 1, 63, 64, 65, 8191, 8193}: the last tile's last wave has 64 (a whole step), 1, 63, 64, 65 elements, or the
last tile lacks one element or holds one, so both kinds of step see steps in which a prefix of the lanes exists, in the leading
(atomic) items as in the trailing (ballot) ones.

Inputs.  The one_digit and distinct_digits constructions of that file at 65 536 + 8192 + 37 (all 1024 elements of a wave on one
counter: a 64-lane same-address atomic; no two lanes of a step alike: every add alone on its counter).  And 4-letter noise with
one 4096-byte block pasted 40 times: from the second pass on the sorted order puts the pasted positions side by side, so the
waves of the middle passes hold runs of one digit, and the lean pass meets runs of equal low words across its tile seams."""
import numpy as np
import pytest

import forward_cases as FC
import oracle_lib as O

import test_packed_pass_lds_gpu as PP
from test_lean_last_pass import TILE

pytestmark = pytest.mark.gpu

SIZES = [PP.PACKED_FROM + extra for extra in (0, 1, 63, 64, 65, 8191, 8193)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alphabet", list(PP.ALPHABETS))
def test_sizes(pkg, alphabet, n):
    x = PP.ALPHABETS[alphabet](n)
    assert x.size == n and n >= PP.PACKED_FROM
    last_wave = (n % TILE) % 1024
    assert last_wave in (0, 1, 63, 64, 65, 1023)
    PP.check_cells(pkg, x, [({"BWTS_VARLEN": "1", "BWTS_KEY_BITS": str(kb)}, None, kb, PP.keys_word(kb, n)) for kb in PP.KEY_BITS])


def test_one_digit(pkg):
    assert PP.N_EXTREME == PP.PACKED_FROM + 8192 + 37
    PP.test_one_digit(pkg)


def test_distinct_digits(pkg):
    PP.test_distinct_digits(pkg)


BLOCK, COPIES = 4096, 40


def pasted_block(n):
    x = FC.noise(n, 4, 13)
    block = x[100:100 + BLOCK].copy()
    starts = 5000 + 4999 * np.arange(COPIES)                  # (apart by more than a block, aligned to nothing)
    assert starts[-1] + BLOCK <= n
    for at in starts:
        x[at:at + BLOCK] = block
    return x, starts


def test_pasted_block(pkg):
    n = 3 * PP.PACKED_FROM + TILE + 37
    x, starts = pasted_block(n)
    assert np.unique(x).size == 4
    # the copies are whole: position p of each holds the same 16 bytes ahead of it (40 equal keys, the last symbols of a copy apart)
    inner = np.arange(BLOCK - 32)
    for at in starts[1:]:
        assert np.array_equal(x[at + inner], x[starts[0] + inner])
    # sorted by their first 2 symbols or more, the 40 copies of a position stand side by side: with 4 letters a 32-bit key prefix
    # is shared by all of them, so from the second pass on a wave's 64 neighbours hold at most two different pasted positions
    assert COPIES * (BLOCK - 32) > n // 2, "most of the input is pasted material"
    PP.check_cells(pkg, x, [({"BWTS_VARLEN": "1", "BWTS_KEY_BITS": str(kb)}, None, kb, PP.keys_word(kb, n)) for kb in PP.KEY_BITS])
