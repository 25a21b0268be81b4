// stage_cut_check.cc -- the cut of a stage call into units (bijective-bwt_amd/csrc/stage_cut.h) as a program of its own, for the
// sanitizers (tests/test_host_layer.py builds it with -fsanitize=address,undefined and runs it as a child process).  The cut is held
// against its serial definition -- the sum over the segments of ceil(len / unit), with its running prefix -- at the units of the three
// stages: move-to-front's tile, the checksum's tile, and the coder's pair of tile and block.  The cuts of a few single inputs are
// printed ("single n mtf-tiles crc-tiles ec-tiles ec-blocks") for the test to compare with the library's plan hooks.
#include "stage_cut.h"

#include <stdio.h>

static int failures = 0, checks = 0;
#define CHECK(cond, ...) do { checks++; if (!(cond)) { failures++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

typedef unsigned long long ull;
static const uint64_t MTF_UNIT = 4096, CRC_UNIT = 65536, EC_TILE = 16384, EC_BLOCK = 262144, EC_TILES_PER_BLOCK = 16;

static uint64_t serial_units(uint64_t len, uint64_t unit) { return len / unit + (len % unit ? 1 : 0); }

// one table (or, with `single`, the one input lengths[0]) at unit_a and, where unit_b is not 0, at unit_b too
static void held_against_serial(const std::vector<uint64_t> &lengths, bool single, uint64_t unit_a, uint64_t unit_b, const char *what)
{
    const uint64_t count = lengths.size();
    std::vector<uint64_t> off(count + 1, 0);
    for (uint64_t s = 0; s < count; s++) off[s + 1] = off[s] + lengths[s];
    const SegMode segs = single ? SEG_SINGLE : SegMode{count};
    const StageCut c = stage_cut_call(off, segs, off[count], unit_a, unit_b);
    CHECK(c.count == count, "%s: count %llu of %llu", what, (ull)c.count, (ull)count);
    const uint64_t unit[2] = {unit_a, unit_b};
    for (int k = 0; k < 2; k++) {
        if (!unit[k]) {
            CHECK(c.first[k].empty() && c.units[k] == 0, "%s: a unit that was not asked for", what);
            continue;
        }
        CHECK(c.first[k].size() == count + 1, "%s, unit %llu: %zu entries for %llu segments", what, (ull)unit[k], c.first[k].size(), (ull)count);
        if (c.first[k].size() != count + 1) continue;
        uint64_t at = 0, wrong = 0;
        for (uint64_t s = 0; s < count; s++) {
            if (c.first[k][s] != at) wrong++;
            at += serial_units(lengths[s], unit[k]);
        }
        CHECK(wrong == 0, "%s, unit %llu: %llu first units differ from the running prefix", what, (ull)unit[k], (ull)wrong);
        CHECK(c.first[k][count] == at && c.units[k] == at, "%s, unit %llu: total %llu, serial %llu", what, (ull)unit[k], (ull)c.units[k], (ull)at);
    }
    if (unit_a == EC_TILE && unit_b == EC_BLOCK && c.first[0].size() == count + 1 && c.first[1].size() == count + 1) {
        uint64_t wrong = 0;
        for (uint64_t s = 0; s < count; s++) {
            const uint64_t tiles = c.first[0][s + 1] - c.first[0][s], blocks = c.first[1][s + 1] - c.first[1][s];
            if (blocks != (tiles + EC_TILES_PER_BLOCK - 1) / EC_TILES_PER_BLOCK) wrong++;
        }
        CHECK(wrong == 0, "%s: %llu segments whose blocks are not ceil(tiles / 16)", what, (ull)wrong);
    }
}

// the lengths around `unit`, cut at (unit_a, unit_b)
static void lengths_around(uint64_t unit, uint64_t unit_a, uint64_t unit_b)
{
    const std::vector<uint64_t> edge = {1, unit - 1, unit, unit + 1, 64 * unit, 64 * unit + 1};
    held_against_serial(edge, false, unit_a, unit_b, "the edge lengths as one table");
    for (uint64_t len : edge) {
        held_against_serial({len}, false, unit_a, unit_b, "a table of one segment");
        held_against_serial({len}, true, unit_a, unit_b, "a single input");
    }
    std::vector<uint64_t> many(4096);
    uint64_t x = 12345;
    for (uint64_t &len : many) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        len = 1 + (x >> 33) % (3 * unit);
    }
    held_against_serial(many, false, unit_a, unit_b, "4096 pseudo-random lengths");
    held_against_serial({(uint64_t)1 << 36}, true, unit_a, unit_b, "a single input of 2^36 bytes");
}

int main()
{
    lengths_around(MTF_UNIT, MTF_UNIT, 0);
    lengths_around(CRC_UNIT, CRC_UNIT, 0);
    lengths_around(EC_TILE, EC_TILE, 0);
    lengths_around(EC_TILE, EC_TILE, EC_BLOCK);
    lengths_around(EC_BLOCK, EC_TILE, EC_BLOCK);
    CHECK(!SEG_SINGLE.table() && SegMode{3}.table() && SegMode{1}.table(), "a table says so");
    CHECK(!SegMode{1}.one_as_single().table() && SegMode{2}.one_as_single().count == 2 && !SEG_SINGLE.one_as_single().table(), "one segment as the single input");
    const uint64_t singles[] = {1, 4095, 4096, 4097, 16384, 16385, 65536, 65537, 262144, 262145, ((uint64_t)1 << 32) + 5, (uint64_t)1 << 36};
    for (uint64_t n : singles) {
        const StageCut ec = stage_cut_single(n, EC_TILE, EC_BLOCK);
        printf("single %llu %llu %llu %llu %llu\n", (ull)n, (ull)stage_cut_single(n, MTF_UNIT).units[0], (ull)stage_cut_single(n, CRC_UNIT).units[0], (ull)ec.units[0],
               (ull)ec.units[1]);
    }
    if (failures) { printf("%d of %d checks FAILED\n", failures, checks); return 1; }
    printf("%d checks ok\n", checks);
    return 0;
}
