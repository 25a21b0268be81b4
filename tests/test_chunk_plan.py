"""CPU suite: the chunk tables of the forward's later rounds as plain arithmetic (bwts_debug_chunk_plan and its sibling with the
target as a parameter: no context, no device).

The tables are reserved once, before the first cut, and every later cut -- the first split of the big list, one append per round, the
re-cut of a compaction at a nominal size of its own -- has to fit them.  They hold a0 / 2048 + 128 entries, because (chunk_rounds.h,
chunk_table_capacity): the store has at most a0 slots in use, a cut of m slots adds ceil(m / S) chunks with S >= 2048, S changes only
at a compaction, which starts the tables over, and fewer than 128 cuts lie between two compactions (rounds are capped).  The tests here
hold that argument against an adversary that plays the driver's bookkeeping with the hook's numbers alone."""
import ctypes
import random

CH_TILE = 2048
CH_CUT_SLACK = 128
TARGET = 16384
MAX_ROUNDS = 81            # the driver fails a run that needs more than 80 rounds after round 0


def nominal(a, target=TARGET):
    s = (a // target + 1023) // 1024 * 1024
    return min(max(s, CH_TILE), 8 * CH_TILE)


def capacity(a0):
    return a0 // CH_TILE + CH_CUT_SLACK


def plan(pkg, a0, a_chunks, target=None):
    out = (ctypes.c_uint64 * 4)()
    if target is None:
        fits = pkg.lib().bwts_debug_chunk_plan(a0, a_chunks, out)
    else:
        fits = pkg.lib().bwts_debug_chunk_plan_target(a0, a_chunks, target, out)
    assert fits in (0, 1)
    return [int(v) for v in out], bool(fits)


def check(pkg, a0, a_chunks, target=None):
    out, fits = plan(pkg, a0, a_chunks, target)
    t = TARGET if target is None else target
    s2 = nominal(a_chunks, t)
    nc = (a_chunks + s2 - 1) // s2
    assert out == [nominal(a0, t), capacity(a0), s2, nc], (a0, a_chunks, out)
    if fits:
        assert out[3] <= out[1], (a0, a_chunks, out)
    return fits


def test_known_pair_is_allowed(pkg):
    # 16334 chunks of 2048: more than the 15072 entries the tables had while they were sized by the first cut's 7168 (that re-cut was
    # refused then); they hold 49 298 now
    out, fits = plan(pkg, 100701917, 33450807)
    assert out == [7168, 49298, 2048, 16334]
    assert fits


def test_every_compaction_fits_the_tables(pkg):
    """An allowed re-cut fits (check), and every re-cut is allowed: none is refused in 120 000 random pairs and at the edges."""
    rng = random.Random(20240607)
    pairs = []
    for _ in range(120000):
        a0 = rng.randrange(65536, 1 << 32)
        pairs.append((a0, rng.randrange(1, a0 // 3 + 1)))
    for a0 in (65536, (1 << 32) - 1):
        pairs += [(a0, 1), (a0, a0 // 3), (a0, a0 // 6), (a0, a0)]
    refused = [(a0, a_chunks) for a0, a_chunks in pairs if not check(pkg, a0, a_chunks)]
    assert not refused, refused[:5]


def test_target_is_the_only_difference(pkg):
    """The old hook is the new one at 16 384; a smaller target raises the nominal sizes and leaves the capacity alone; targets outside
    16 .. 16 384 are refused."""
    rng = random.Random(7)
    for _ in range(2000):
        a0 = rng.randrange(65536, 1 << 32)
        a_chunks = rng.randrange(1, a0 + 1)
        assert plan(pkg, a0, a_chunks) == plan(pkg, a0, a_chunks, TARGET)
        for target in (16, 64, 1000, 16383):
            assert check(pkg, a0, a_chunks, target)
    assert plan(pkg, 1 << 21, 140013, 64)[0] == [16384, 1152, 3072, 46]
    out = (ctypes.c_uint64 * 4)()
    for bad in (0, 15, 16385, 1 << 20):
        assert pkg.lib().bwts_debug_chunk_plan_target(1 << 21, 1000, bad, out) == -1


class Tables:
    """The driver's bookkeeping (chunk_rounds in csrc/chunk_rounds.h) with the hook's numbers and nothing else: the first cut, the
    first split of the big list, per round an append of what leaves it, and the compaction rule.  `cap` may be overridden to play the
    same run against another capacity; the first cut that does not fit it is then kept in `overrun`, not asserted.  With the hook's own
    capacity every step asserts nchunks <= capacity, and always that the store holds at most a0 slots."""

    def __init__(self, pkg, a0, target, cap=None):
        self.pkg, self.a0, self.target = pkg, a0, target
        (self.S, hook_cap, _, _), _ = plan(pkg, a0, a0, target)
        self.cap = hook_cap if cap is None else cap
        self.nchunks = self.tail = self.a_chunks = self.big = 0
        self.peak = self.compactions = self.rounds = 0
        self.strict, self.overrun = cap is None, None

    def cut(self, m, what):
        self.nchunks += -(-m // self.S)
        self.tail += m
        self.peak = max(self.peak, self.nchunks)
        assert self.tail <= self.a0, (what, self.a0, self.tail)
        if self.strict:
            assert self.nchunks <= self.cap, (what, self.a0, self.target, self.rounds, self.nchunks, self.cap)
        elif self.nchunks > self.cap and self.overrun is None:
            self.overrun = (what, self.rounds, self.nchunks)

    def start(self, a_small, mid):
        """a_small elements in groups of at most 256, mid in groups of 257 .. 2048 (they leave the big list at once), the rest stays"""
        assert a_small + mid <= self.a0
        if a_small:
            self.cut(a_small, "first cut")
        if mid:
            self.cut(mid, "first split")
        self.a_chunks = a_small + mid
        self.big = self.a0 - a_small - mid

    def trip(self, moves):
        """One host round trip: moves = [(elements still tied in chunks, elements leaving the big list, elements staying in it)] per
        round (one round while the big list holds anything, else two), then the compaction rule."""
        assert len(moves) == (1 if self.big else 2)
        for in_chunks, leaves, stays in moves:
            assert in_chunks <= self.a_chunks and leaves + stays <= self.big
            self.rounds += 1
            if leaves:
                self.cut(leaves, "append")
            self.big = stays
            self.a_chunks = in_chunks + leaves
        if self.nchunks >= 64 and self.a_chunks > 0 and 3 * self.a_chunks < self.tail:
            (_, _, S2, nc), fits = plan(self.pkg, self.a0, self.a_chunks, self.target)
            assert fits, ("a re-cut was refused", self.a0, self.a_chunks, self.target)
            self.compactions += 1
            self.S, self.nchunks, self.tail = S2, 0, 0
            self.cut(self.a_chunks, "re-cut")
            assert self.nchunks == nc


def worst_schedule(pkg, a0, target=TARGET, cap=None):
    """The schedule built against the tables: a first cut of just 64 chunks, which round 1 empties to one element, so that the list is
    compacted as early as the rule allows and to the smallest nominal size; then everything else leaves the big list in equal pieces of
    whole tiles plus one element, one per round, each of which ends in a ragged chunk."""
    t = Tables(pkg, a0, target, cap)
    a_small = 63 * t.S + 1
    t.start(a_small, 0)
    assert t.nchunks == 64
    t.trip([(1, 0, t.big)])
    assert t.compactions == 1 and t.S == CH_TILE and t.nchunks == 1
    left = MAX_ROUNDS - t.rounds
    while t.big:
        piece = t.big if left == 1 else min(t.big, (t.big // left) // CH_TILE * CH_TILE + 1)
        t.trip([(t.a_chunks, piece, t.big - piece)])
        left -= 1
    assert t.rounds == MAX_ROUNDS and t.tail == a0 - a_small + 1
    return t


def test_worst_schedule_fits(pkg):
    rng = random.Random(11)
    for a0 in [4 * 1024 * 1024, 85739813, 1 << 29, (1 << 32) - 1] + [rng.randrange(1 << 22, 1 << 32) for _ in range(200)]:
        t = worst_schedule(pkg, a0)
        # it comes within the slack of the capacity: the bound is not loose
        assert t.cap - CH_CUT_SLACK - 64 * (8 * CH_TILE // CH_TILE) <= t.peak <= t.cap, (a0, t.peak, t.cap)
    for a0 in [1 << 20, (1 << 21) + 5, 1 << 22] + [rng.randrange(1 << 20, 1 << 26) for _ in range(200)]:
        for target in (16, 64, 1024):
            if 63 * nominal(a0, target) + 1 < a0:
                worst_schedule(pkg, a0, target)


def test_worst_schedule_overran_the_first_cuts_capacity(pkg):
    """Sized by the first cut's nominal size the tables had a0 // S(a0) + 1024 entries, and the worst schedule overran them.  For
    a0 = 85 739 813 (S = 6144): 14 979 entries; the worst schedule makes 41 757 chunks and passes that capacity with the append of round
    30 (15 135 chunks); the tables hold 41 993 now.  For a0 = 254 419 860 (S = 16 384: the tied list of the suffix sort over the byte
    planes of a smooth float32 field of 2^29 bytes, which ended in "chunk table full"): 16 552 entries against 123 805 chunks, passed in
    round 12 (17 018 chunks); they hold 124 356 now."""
    for a0, S, old_cap, peak, cap, overrun in ((85739813, 6144, 14979, 41757, 41993, ("append", 30, 15135)),
                                               (254419860, 16384, 16552, 123805, 124356, ("append", 12, 17018))):
        assert nominal(a0) == S and a0 // nominal(a0) + 1024 == old_cap
        t = worst_schedule(pkg, a0)
        assert (t.peak, t.cap) == (peak, cap) and t.overrun is None
        assert worst_schedule(pkg, a0, cap=old_cap).overrun == overrun


def test_random_schedules_fit(pkg):
    rng = random.Random(20250101)
    for i in range(3000):
        a0 = rng.randrange(65536, 1 << 32) if i % 3 else rng.randrange(65536, 1 << 24)
        target = TARGET if i % 2 else rng.choice((16, 64, 256, 4096))
        t = Tables(pkg, a0, target)
        a_small = rng.randrange(0, a0 + 1) if rng.random() < 0.7 else min(a0, rng.randrange(0, 80) * t.S + rng.randrange(0, 3))
        mid = rng.randrange(0, a0 - a_small + 1) if rng.random() < 0.5 else 0
        t.start(a_small, mid)
        shrink = rng.choice((0.0, 0.01, 0.3, 0.9, 1.0))              # the share of the chunks' elements that a round leaves tied
        drain = rng.choice((0.0, 0.05, 0.5, 1.0))                    # the share of the big list that leaves per round, at most
        while t.rounds < MAX_ROUNDS - 1 and (t.a_chunks or t.big):
            moves = []
            a_chunks, big = t.a_chunks, t.big
            for _ in range(1 if t.big else 2):
                in_chunks = min(a_chunks, int(a_chunks * shrink * rng.random() * 2))
                leaves = min(big, int(big * drain * rng.random()) + (rng.randrange(0, 3 * CH_TILE) if rng.random() < 0.5 else 0))
                stays = rng.randrange(0, big - leaves + 1) if rng.random() < 0.1 else big - leaves
                moves.append((in_chunks, leaves, stays))
                a_chunks, big = in_chunks + leaves, stays
            t.trip(moves)
