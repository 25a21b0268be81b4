"""CPU suite: the chunk tables of the forward's later rounds as plain arithmetic (bwts_debug_chunk_plan: no context, no device).

A compaction re-cuts the elements left in chunks by their own nominal size; the tables were sized once, for the whole tied list.
The nominal size is rounded up to whole K, so the tables may hold as few as about 15 K chunks while a re-cut makes up to 16 K:
the compaction must be refused whenever its chunks would not fit."""
import ctypes
import random

CH_TILE = 2048


def nominal(a):
    s = (a // 16384 + 1023) // 1024 * 1024
    return min(max(s, CH_TILE), 8 * CH_TILE)


def capacity(a0):
    return a0 // nominal(a0) + 1024


def plan(pkg, a0, a_chunks):
    out = (ctypes.c_uint64 * 4)()
    allowed = pkg.lib().bwts_debug_chunk_plan(a0, a_chunks, out)
    assert allowed in (0, 1)
    return list(out), bool(allowed)


def check(pkg, a0, a_chunks):
    out, allowed = plan(pkg, a0, a_chunks)
    s2 = nominal(a_chunks)
    nc = (a_chunks + s2 - 1) // s2
    assert out == [nominal(a0), capacity(a0), s2, nc], (a0, a_chunks, out)
    if allowed:
        assert out[3] <= out[1], (a0, a_chunks, out)
    return allowed


def test_known_overrun_pair_is_refused(pkg):
    # 16334 chunks of 2048 against tables of 15072 entries
    out, allowed = plan(pkg, 100701917, 33450807)
    assert out == [7168, 15072, 2048, 16334]
    assert not allowed


def test_allowed_compactions_fit_the_tables(pkg):
    rng = random.Random(20240607)
    allowed = refused = 0
    pairs = []
    for _ in range(120000):
        a0 = rng.randrange(65536, 1 << 32)
        pairs.append((a0, rng.randrange(1, a0 // 3 + 1)))
    for a0 in (65536, (1 << 32) - 1):
        pairs += [(a0, 1), (a0, a0 // 3), (a0, a0 // 6)]
    for a0, a_chunks in pairs:
        if check(pkg, a0, a_chunks):
            allowed += 1
        else:
            refused += 1
    # nearly every compaction is allowed: the refusal is a guard, not a policy
    assert refused * 100 < allowed
