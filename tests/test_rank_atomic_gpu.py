"""GPU suite (-m gpu): the hardware behaviour the split ranking of the packed radix passes rests on (csrc/device_utils.h,
wave_rank_atomic_step; csrc/radix.hip, rank_split): the lanes of one returning LDS add that name the same address are served in
lane order, and a wave's LDS instructions run in program order, so an item's returned value is the number of earlier
(item, lane) pairs of its wave with its digit -- the rank the ballot step computes.

bwts_debug_rank_steps runs rank_split in one workgroup (8 waves, sixteen items a lane) over digits and validity bytes given here and
returns every item's rank; expected() is the same count in numpy.  Every pattern runs with all sixteen items atomic (the step
alone), with none (the ballot step on the same u32 counters) and with each split the passes are built with, where atomic and
ballot steps share the counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVES, ITEMS, LANES = 8, 16, 64
INVALID = 0xFFFFFFFF


def expected(d, v):
    """rank = number of earlier (item, lane) pairs of the wave with the same digit, valid items only."""
    want = np.full(d.shape, INVALID, dtype=np.uint32)
    for w in range(WAVES):
        dw, vw = d[w].reshape(-1), v[w].reshape(-1).astype(bool)
        seen = np.zeros(256, dtype=np.int64)
        out = want[w].reshape(-1)
        for i in np.flatnonzero(vw):
            out[i] = seen[dw[i]]
            seen[dw[i]] += 1
    return want


def prefix_valid(lanes):
    """Every step whole but the last, whose first `lanes` lanes exist."""
    v = np.ones((WAVES, ITEMS, LANES), dtype=np.uint8)
    v[:, -1, lanes:] = 0
    return v


def patterns():
    rng = np.random.default_rng(2024)
    shape = (WAVES, ITEMS, LANES)
    lane = np.broadcast_to(np.arange(LANES), shape)
    item = np.broadcast_to(np.arange(ITEMS)[None, :, None], shape)
    ones = np.ones(shape, dtype=np.uint8)
    out = {
        "all_equal": (np.full(shape, 37), ones),
        "two_by_lane": (np.where(lane % 2 == 0, 5, 250), ones),
        "two_by_item": (np.where(item % 2 == 0, 5, 250), ones),
        # 64 distinct digits in every step, another window of the 256 from step to step and wave to wave
        "distinct_per_step": ((lane * 3 + item * 17 + np.arange(WAVES)[:, None, None] * 29) % 256, ones),
    }
    for values in (256, 4, 2):
        out["random_%d" % values] = (rng.integers(0, values, size=shape), ones)
    for lanes in (0, 1, 63, 64):
        out["valid_prefix_%d" % lanes] = (rng.integers(0, 4, size=shape), prefix_valid(lanes))
    # (one more shape of validity: a wave's tail past the array's end, whole steps missing)
    v = np.ones(shape, dtype=np.uint8)
    v[-1, 9, 17:] = 0
    v[-1, 10:] = 0
    out["wave_tail"] = (rng.integers(0, 3, size=shape), v)
    return {k: (np.ascontiguousarray(d, dtype=np.uint8), v) for k, (d, v) in out.items()}


PATTERNS = patterns()
WANT = {k: expected(d, v) for k, (d, v) in PATTERNS.items()}


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(0) as c:
        yield c


def check(ctx, name, k):
    d, v = PATTERNS[name]
    got, _ = ctx.debug_rank_steps(d, v, k)
    bad = np.argwhere(got != WANT[name])
    assert bad.size == 0, (name, k, "first wrong (wave, item, lane):", bad[:4].tolist(),
                           [(int(got[tuple(b)]), int(WANT[name][tuple(b)])) for b in bad[:4]])


@pytest.mark.parametrize("name", list(PATTERNS))
def test_atomic_step_alone(ctx, name):
    """Sixteen atomic items: lane-order service inside an instruction, program order between instructions."""
    check(ctx, name, ITEMS)


@pytest.mark.parametrize("name", list(PATTERNS))
def test_ballot_step_on_u32_counters(ctx, name):
    check(ctx, name, 0)


@pytest.mark.parametrize("name", list(PATTERNS))
def test_shipped_split(ctx, name):
    """The mixtures the passes are built with: the atomic items' adds and the ballot items' read and write share one counter."""
    _, shipped = ctx.debug_rank_steps(*PATTERNS[name], 0)
    assert len(shipped) == 4 and all(0 <= k <= ITEMS and k % 2 == 0 for k in shipped), shipped
    for k in sorted(set(shipped) | {2, 14}):           # (and the two most lopsided splits)
        check(ctx, name, k)


def test_expected_is_what_the_issue_states():
    """The numpy reference on a case small enough to state by hand: wave 0, digits 7 7 9 7 in lanes 0 .. 3 of item 0, 7 in lane 0 of item 1."""
    d = np.zeros((WAVES, ITEMS, LANES), dtype=np.uint8)
    v = np.zeros_like(d)
    d[0, 0, :4] = [7, 7, 9, 7]
    v[0, 0, :4] = 1
    d[0, 1, 0], v[0, 1, 0] = 7, 1
    want = expected(d, v)
    assert want[0, 0, :4].tolist() == [0, 1, 0, 2] and want[0, 1, 0] == 3
    assert (want[v == 0] == INVALID).all()


def test_bad_arguments(ctx):
    d, v = PATTERNS["all_equal"]
    for k in (-1, 3, 17):
        with pytest.raises(Exception):
            ctx.debug_rank_steps(d, v, k)
