// stage_cut.h -- how a call of a stage behind the transform (mtf.hip, ec.hip, crc.hip) is cut into units: every segment on its own,
// rounded up to whole units, the segments' units numbered one after the other over the call.  Plain C++ with no device runtime, like
// copy_pool.h and seg_layout.h; tests/stage_cut_check.cc holds it against the serial definition.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <vector>

// Which input a stage works on: one input of n bytes (count == 0), or the `count` segments of the context's table.
struct SegMode {
    uint64_t count;
    bool table() const { return count != 0; }
    // move-to-front's rule: a table of one segment runs as the single-input call
    SegMode one_as_single() const { return SegMode{count > 1 ? count : 0}; }
};
static const SegMode SEG_SINGLE = {0};

// first[k][s]: the first unit of size unit[k] of segment s, counted over the call; count + 1 entries, so first[k][s + 1] - first[k][s]
// is what segment s has and units[k] == first[k][count] the call's total.  first[1] stays empty where one unit size was asked for.
struct StageCut {
    uint64_t count, units[2];
    std::vector<uint64_t> first[2];
};

// off: count + 1 offsets, the context's table or {0, n} for one input
static inline StageCut stage_cut(const uint64_t *off, uint64_t count, uint64_t unit_a, uint64_t unit_b = 0)
{
    StageCut c;
    c.count = count;
    const uint64_t unit[2] = {unit_a, unit_b};
    for (int k = 0; k < 2; k++) {
        c.units[k] = 0;
        if (!unit[k]) continue;
        c.first[k].resize((size_t)count + 1);
        for (uint64_t s = 0; s < count; s++) {
            c.first[k][(size_t)s] = c.units[k];
            c.units[k] += (off[s + 1] - off[s] + unit[k] - 1) / unit[k];
        }
        c.first[k][(size_t)count] = c.units[k];
    }
    return c;
}

static inline StageCut stage_cut_single(uint64_t n, uint64_t unit_a, uint64_t unit_b = 0)
{
    const uint64_t one[2] = {0, n};
    return stage_cut(one, 1, unit_a, unit_b);
}

// the cut of a call: of the table's segments (seg_off: its count + 1 offsets), or of the one input of n bytes
static inline StageCut stage_cut_call(const std::vector<uint64_t> &seg_off, SegMode segs, uint64_t n, uint64_t unit_a, uint64_t unit_b = 0)
{
    return segs.table() ? stage_cut(seg_off.data(), segs.count, unit_a, unit_b) : stage_cut_single(n, unit_a, unit_b);
}
