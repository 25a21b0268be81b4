"""CPU model of the plane-cost estimate (include/bwts_members.h, "The estimate"; bijective-bwt_amd/csrc/estimate_plan.h): what the order-0
coder would make of a member's byte planes as they are, and of the planes of its delta-filtered elements.  Exact integer arithmetic in
Python integers, lg included; numpy only counts the bytes.  The device, the host and this file agree bit for bit."""
import numpy as np

import delta_model as D

LOG_UNIT = 18
UNIT = 1 << LOG_UNIT                # elements of a unit: what one 256 KiB coder block of a plane spans
FRAC = 16                           # fraction bits of lg
MARGIN_SHIFT = 6                    # a filter must save more than 1/64 of the unfiltered estimate


def lg(x):
    """Fixed-point log2 of an integer 1 <= x < 2^32, 16 fraction bits: normalise, then sixteen squarings."""
    assert 1 <= x < 1 << 32
    k = x.bit_length() - 1
    y = x << (31 - k)
    r = k
    for _ in range(FRAC):
        y = (y * y) >> 31
        r <<= 1
        if y >> 32:
            y >>= 1
            r |= 1
    return r


def term(c):
    return c * lg(c) if c else 0


def hist_bytes(counts):
    """The bytes of one unit's plane from its 256 counts."""
    counts = [int(c) for c in counts]
    bits = max(0, term(sum(counts)) - sum(term(c) for c in counts))
    return (bits + (8 << FRAC) - 1) >> (3 + FRAC)


def units(ln, w):
    """The units of a member of ln bytes and width w: none where it has no whole element."""
    return (ln // w + UNIT - 1) >> LOG_UNIT


def _planes_bytes(x, w, q):
    """The sum over units and planes for the q elements of width w at the start of the bytes x."""
    planes = x[:q * w].reshape(q, w)
    total = 0
    for e0 in range(0, q, UNIT):
        for p in range(w):
            total += hist_bytes(np.bincount(planes[e0:e0 + UNIT, p], minlength=256))
    return total


def estimate(member, w):
    """(est_none, est_delta) of one member."""
    assert w in D.WIDTHS
    x = D._u8(member)
    q = x.size // w
    if q == 0:
        return 0, 0
    return _planes_bytes(x, w, q), _planes_bytes(D._u8(D.encode(x, w)), w, q)


def estimate_members(members, widths=None):
    """bwts_members_estimate: two lists."""
    widths = [1] * len(members) if widths is None else widths
    both = [estimate(m, w) for m, w in zip(members, widths)]
    return [b[0] for b in both], [b[1] for b in both]


def choose_filter(est_none, est_delta):
    """The writer's rule for a filter left open: delta iff it saves more than 1/64 of the unfiltered estimate."""
    return D.FILTER_DELTA if est_delta + (est_none >> MARGIN_SHIFT) < est_none else D.FILTER_NONE
