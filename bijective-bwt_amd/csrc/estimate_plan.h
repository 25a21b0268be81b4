// estimate_plan.h -- the arithmetic of the plane-cost estimate (include/bwts_members.h, "The estimate") that host and
// device share: the units a member is cut into, the fixed-point logarithm, the cost of one histogram, the serial statement of the whole
// estimate and the rule that makes a filter of two estimates.  Exact integer arithmetic, no floating point anywhere: the kernel of
// estimate.hip, the host side of the calls, tests/estimate_model.py (the same statements in Python integers) and a stand-alone host
// program (tests/estimate_plan_check.cc, built with the sanitizers) agree bit for bit.
//
// A member of len bytes and width w has q = len / w elements; the tail of len - q w bytes is copied under either filter and is not
// counted.  The member is cut into units of ESTIMATE_UNIT = 2^18 elements: the elements that one 256 KiB coder block of a plane spans.
// For every unit, every plane p < w and both filters, c[0..255] is the histogram of byte p of the unit's elements -- filter 0: the
// element itself; filter 1: zigzag(element - predecessor) at width w as delta_plan.h has it, the predecessor of a member's first element
// being 0 and that of a unit's first element the last element of the unit before.  With N the sum of c,
//     bits  = N lg(N) - sum of c[s] lg(c[s])        (0 where the subtraction would go below it)
//     bytes = ceil(bits / (8 * 2^16))
// and a member's estimate under a filter is the sum of `bytes` over its units and planes.  q = 0: both estimates are 0.
#pragma once
#include "delta_plan.h"

#define ESTIMATE_LOG_UNIT 18u                        // elements of a unit: a coder block (EC_K tiles of 2^EC_LOG_T bytes) of one plane
#define ESTIMATE_UNIT (1u << ESTIMATE_LOG_UNIT)
#define ESTIMATE_UNIT_TILES (ESTIMATE_UNIT >> PLANES_LOG_E)     // delta.hip's tiles to a unit
#define ESTIMATE_FRAC 16u                            // fraction bits of lg
#define ESTIMATE_MARGIN_SHIFT 6u                     // a filter must save more than 1/64 of the unfiltered estimate

// units of a member: ceil(q / 2^18), none where it has no whole element; unit j holds the elements [j 2^18, min((j + 1) 2^18, q))
PLANES_HD uint64_t estimate_units(uint64_t len, uint32_t w)
{
    return (delta_q(len, w) + ESTIMATE_UNIT - 1u) >> ESTIMATE_LOG_UNIT;
}
PLANES_HD uint32_t estimate_unit_elems(uint64_t len, uint32_t w, uint64_t j)
{
    const uint64_t q = delta_q(len, w), e0 = j << ESTIMATE_LOG_UNIT;
    return e0 >= q ? 0u : (q - e0 < ESTIMATE_UNIT ? (uint32_t)(q - e0) : ESTIMATE_UNIT);
}
// first[s]: the first unit of member s over the call, count + 1 entries (a member without elements has none: its first is its
// neighbour's); the total is first[count].  take: null, or a byte per member, zero for a member that is left out (it gets no unit).
PLANES_HD uint64_t estimate_cut(const uint64_t *off, const uint32_t *widths, const uint8_t *take, uint64_t count, uint64_t *first)
{
    uint64_t units = 0;
    for (uint64_t s = 0; s < count; s++) {
        first[s] = units;
        if (!take || take[s]) units += estimate_units(off[s + 1] - off[s], widths[s]);
    }
    first[count] = units;
    return units;
}

// lg(x) = floor(2^16 log2(x)) or one less, for 1 <= x < 2^32: the integer part is the place k of x's highest bit; x is normalised to
// y = x 2^(31 - k) in [2^31, 2^32), 1.0 <= y / 2^31 < 2.0, and sixteen times y becomes y^2 / 2^31 (rounded down), which yields the next
// fraction bit: 1, and y halved (rounded down), where the square reached 2.0.  lg(2^k) = k 2^16; lg never decreases as x grows.
PLANES_HD uint32_t estimate_lg(uint32_t x)
{
    uint32_t k = 0;
    while ((x >> k) > 1u) k++;
    uint64_t y = (uint64_t)x << (31u - k);
    uint32_t r = k;
    for (uint32_t i = 0; i < ESTIMATE_FRAC; i++) {
        y = (y * y) >> 31;
        r <<= 1;
        if (y >> 32) { y >>= 1; r |= 1u; }
    }
    return r;
}
// one term of a cost: c lg(c), 0 for c = 0; c <= 2^18 in a unit, so a term is below 2^18 * 18 * 2^16 < 2^39 and 256 of them cannot wrap
PLANES_HD uint64_t estimate_term(uint32_t c) { return c ? (uint64_t)c * estimate_lg(c) : 0u; }
// the bytes of a histogram of N entries whose terms add up to `terms`
PLANES_HD uint64_t estimate_bytes(uint32_t N, uint64_t terms)
{
    const uint64_t all = estimate_term(N), bits = all > terms ? all - terms : 0u;
    return (bits + ((8ull << ESTIMATE_FRAC) - 1u)) >> (3u + ESTIMATE_FRAC);
}
PLANES_HD uint64_t estimate_hist_bytes(const uint32_t c[256])
{
    uint32_t N = 0;
    uint64_t terms = 0;
    for (int s = 0; s < 256; s++) { N += c[s]; terms += estimate_term(c[s]); }
    return estimate_bytes(N, terms);
}

// the serial statement: est[0], est[1] of the member of len bytes at m
PLANES_HD void estimate_serial(const uint8_t *m, uint64_t len, uint32_t w, uint64_t est[2])
{
    const uint64_t q = delta_q(len, w), mask = delta_mask(w);
    est[0] = est[1] = 0;
    uint64_t prev = 0;
    for (uint64_t e0 = 0; e0 < q; e0 += ESTIMATE_UNIT) {
        const uint64_t e1 = q - e0 < ESTIMATE_UNIT ? q : e0 + ESTIMATE_UNIT;
        for (uint32_t p = 0; p < w; p++) {
            uint32_t c[2][256];
            for (int s = 0; s < 256; s++) c[0][s] = c[1][s] = 0;
            uint64_t pr = prev;
            for (uint64_t i = e0; i < e1; i++) {
                const uint64_t a = delta_load(m + i * w, w);
                c[0][(a >> (8u * p)) & 255u]++;
                c[1][(delta_zigzag((a - pr) & mask, w) >> (8u * p)) & 255u]++;
                pr = a;
            }
            est[0] += estimate_hist_bytes(c[0]);
            est[1] += estimate_hist_bytes(c[1]);
        }
        prev = delta_load(m + (e1 - 1u) * w, w);
    }
}

// The writer's rule for a filter left open (BWTS_FILTER_AUTO): delta iff it saves more than 1/64 of the unfiltered estimate -- a filter
// that buys nothing costs a decode sweep, and noise must not get one by chance.
PLANES_HD uint32_t estimate_filter(uint64_t est_none, uint64_t est_delta)
{
    return est_delta + (est_none >> ESTIMATE_MARGIN_SHIFT) < est_none ? DELTA_FILTER_DELTA : DELTA_FILTER_NONE;
}
