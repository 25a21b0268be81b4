"""GPU suite (-m gpu): the shared pass of the segmented inverse -- one splitter walk over a run of segments (plan B of
bwts_inverse_segments) -- against the CPU oracle per segment, the engine's own reports (Context.debug_segments_report,
Context.debug_inverse_report) and the segmented model (tests/segment_inverse_model.py).  Exact bytes and counts; no tolerance.

The shapes are the smallest at which the pass can go wrong: below 2^28 elements the engine picks g = 4 (a splitter every 16 positions,
slots of 64 symbols), so segment starts fall off the 16-grid, segments of 15 / 16 / 17 and 63 / 64 / 65 bytes sit around both sizes,
and segments of 1 .. 5 bytes hold no splitter at all.  Every context is made fresh under its knobs (a context reads them when it is
made), BWTS_TEST_KNOBS=1 and BWTS_POISON=1.  BWTS_SEG_INV_PLAN=shared forces the plan only: which segments are long enough to go
single stays the cost estimate's choice (it sends a 300 000-byte segment among short ones alone), so the tests that want a whole set in
one pass also set BWTS_SEG_INV_BIG above every length (ALL)."""
import contextlib
import os
import time

import numpy as np
import pytest

import inverse_cases as IC
import inverse_model as M
import oracle_lib as O
import segment_cases as C
import segment_inverse_model as SM

pytestmark = pytest.mark.gpu

_KNOBS = ("BWTS_TEST_KNOBS", "BWTS_POISON", "BWTS_SPLIT_LOG2", "BWTS_INV_MARK", "BWTS_BYTEMARK", "BWTS_FORCE_WIDE", "BWTS_SEG_INV_PLAN",
          "BWTS_SEG_INV_BIG")


@contextlib.contextmanager
def fresh_context(pkg, plan=None, big=None, g=None, mark=None):
    saved = {k: os.environ.get(k) for k in _KNOBS}
    try:
        for k in _KNOBS:
            os.environ.pop(k, None)
        os.environ.update(BWTS_TEST_KNOBS="1", BWTS_POISON="1")
        for k, v in (("BWTS_SEG_INV_PLAN", plan), ("BWTS_SEG_INV_BIG", big), ("BWTS_SPLIT_LOG2", g), ("BWTS_INV_MARK", mark)):
            if v is not None:
                os.environ[k] = str(v)
        with pkg.Context(0) as ctx:
            yield ctx
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


ALL = 1 << 32        # BWTS_SEG_INV_BIG: no segment is long enough to go single


@pytest.fixture(scope="module")
def shared_ctx(pkg):
    """One context with the shared plan forced for every segment, for the tests that need no other knob."""
    with fresh_context(pkg, plan="shared", big=ALL) as ctx:
        yield ctx


def _all_shared(rep, lengths):
    return rep["plan"] == "shared" and rep["runs"] == 1 and (rep["shared_segments"], rep["shared_bytes"]) == (len(lengths), int(np.sum(lengths))) and \
        (rep["lane_segments"], rep["lane_bytes"], rep["single_segments"], rep["single_bytes"]) == (0, 0, 0, 0)


# ---- boundaries --------------------------------------------------------------------------------------------------------------------

BOUNDARY = np.array([1, 15, 16, 17, 63, 64, 65, 4097, 1, 300000, 5, 2, 70001], dtype=np.uint64)
_boundary = {}


def boundary(kind):
    """(x, the oracle's inverse of x per segment, its factor count) -- computed once per kind and left unchanged."""
    if kind not in _boundary:
        x = O.generate(kind, int(BOUNDARY.sum()), 23)
        want = C.expected_inverse(x, BOUNDARY)
        for a in (x, want):
            a.setflags(write=False)
        _boundary[kind] = (x, want, C.expected_factors(want, BOUNDARY))
    return _boundary[kind]


@pytest.mark.parametrize("kind", ["zipf", "text", "dna"])
def test_boundaries(shared_ctx, kind):
    ctx = shared_ctx
    x, want, factors = boundary(kind)
    y = ctx.forward_segments(x, BOUNDARY)
    back = ctx.inverse_segments(y, BOUNDARY)
    t, rep, last = ctx.timings(), ctx.debug_segments_report(), ctx.debug_inverse_report()[-1]
    assert np.array_equal(back, x)
    assert _all_shared(rep, BOUNDARY), rep
    assert t.n == x.size and t.factors == C.expected_factors(x, BOUNDARY) and rep["attempts"] == t.attempts
    assert last["form"] == "segmented" and last["outcome"] == "DONE" and last["g"] == 4, last
    got = ctx.inverse_segments(x, BOUNDARY)                    # raw bytes as an inverse input: each segment against the oracle
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert ctx.timings().factors == factors


@pytest.mark.parametrize("big,singles", [(65536, [300000, 70001]), (131072, [300000])])
def test_runs_with_a_nonzero_base(pkg, big, singles):
    """BWTS_SEG_INV_BIG cuts the set: the segments of `big` bytes or more go single and split the rest into runs whose indices are
    rebased.  (Of the boundary set 70 001 is also above 65 536: two single segments there, one at 131 072; two runs at both.)"""
    x, want, factors = boundary("text")
    ls = [int(v) for v in BOUNDARY]
    assert [v for v in ls if v >= big] == singles
    with fresh_context(pkg, plan="shared", big=big) as ctx:
        got = ctx.inverse_segments(x, BOUNDARY)
        t, rep = ctx.timings(), ctx.debug_segments_report()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert t.factors == factors
    assert rep["plan"] == "shared" and rep["big"] == big and rep["runs"] == 2, rep
    assert (rep["single_segments"], rep["single_bytes"]) == (len(singles), sum(singles)), rep
    assert (rep["shared_segments"], rep["shared_bytes"]) == (len(ls) - len(singles), sum(ls) - sum(singles)), rep
    assert (rep["lane_segments"], rep["lane_bytes"]) == (0, 0), rep


def test_host_entry_in_place_and_device_entry(shared_ctx):
    ctx = shared_ctx
    x, want, factors = boundary("zipf")
    buf = x.copy()
    out = ctx.inverse_segments(buf, BOUNDARY, out=buf)             # out is in
    assert out is buf and np.array_equal(buf, want)
    n = x.size
    d_in, d_out = ctx.alloc(n), ctx.alloc(n)
    try:
        d_in.upload(x)
        ctx.inverse_segments_device(d_in, BOUNDARY, d_out)
        assert _all_shared(ctx.debug_segments_report(), BOUNDARY)
        assert ctx.timings().factors == factors
        assert np.array_equal(d_out.download(), want)
        assert np.array_equal(d_in.download(), x)                  # the input is read, not written
    finally:
        d_in.free()
        d_out.free()


# ---- segments that share material ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_structured_families_both_directions(shared_ctx, name):
    """Copies place equal cycle structures in many segments; the periodic sets are Theta(n) cycles without a splitter."""
    ctx = shared_ctx
    data, lengths = C.build(name)
    y = ctx.forward_segments(data, lengths)
    back = ctx.inverse_segments(y, lengths)
    rep = ctx.debug_segments_report()
    assert np.array_equal(back, data)
    assert ctx.timings().factors == C.expected_factors(data, lengths)
    assert rep["plan"] == "shared" and rep["shared_bytes"] + rep["single_bytes"] == data.size and rep["lane_bytes"] == 0, rep
    want = C.expected_inverse(data, lengths)
    got = ctx.inverse_segments(data, lengths)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert ctx.timings().factors == C.expected_factors(want, lengths)


def test_tiny_segments_against_the_table(shared_ctx):
    """200 000 segments of 1 .. 3 bytes: every cycle is one without a splitter, across thousands of segment boundaries."""
    data, lengths = C.tiny_segments(31, 200000)
    table = C.TinyTable(O.inverse)
    want = table.apply(data, lengths)
    got = shared_ctx.inverse_segments(data, lengths)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert shared_ctx.timings().factors == table.count_factors(want, lengths)
    assert _all_shared(shared_ctx.debug_segments_report(), lengths)


# ---- the inverse's built inputs side by side ---------------------------------------------------------------------------------------

SIDE_BY_SIDE = ["rot2k-c2odd", "short-l20-w600", "sorted-above", "rot-c2624-g4", "cycles-r15"]
_sets = {}


def built_set(which):
    """(data, lengths, the oracle's inverse per segment, the segmented model), built once.  "side": the built inputs with a 300 000-byte
    text between them.  "overflow": rot-c2624-g4 between two short texts -- in so short a run its virtual nodes overflow the node pool,
    which the side-by-side run (a pool sized for 4.3 M elements) holds."""
    if which not in _sets:
        by = {c.name: c for c in IC.CASES}
        if which == "side":
            segs = []
            for i, name in enumerate(SIDE_BY_SIDE):
                if i:
                    segs.append(O.generate("text", 300000, 11))
                segs.append(np.ascontiguousarray(by[name].build(), dtype=np.uint8))
        else:
            segs = [O.generate("text", 4097, 12), np.ascontiguousarray(by["rot-c2624-g4"].build(), dtype=np.uint8), O.generate("text", 33, 13)]
        data, lengths = np.concatenate(segs), np.array([s.size for s in segs], dtype=np.uint64)
        want = C.expected_inverse(data, lengths)
        for a in (data, want):
            a.setflags(write=False)
        _sets[which] = (data, lengths, want, SM.SegmentModel(data, lengths))
    return _sets[which]


def check_pass_report(mod, g, mark, rep, t):
    """The records of the pass's attempts against the segmented model, and the chain against what the counts decide."""
    assert t.attempts == len(rep) and rep, rep
    for a in rep:
        ma = mod.at(a["g"])
        assert a["form"] == "segmented" and a["s"] == ma["s"] and a["node_cap"] == ma["s"] + ma["room"], (a, ma)
        a["overflow"] = a["outcome"] == "RETRY_DENSE" and a["virtual"] > ma["room"]
        assert a["overflow"] == ma["overflow"], (a, ma)
        if not ma["overflow"]:
            assert a["virtual"] == ma["virtual"], (a, ma)
    last, ml = rep[-1], mod.at(rep[-1]["g"])
    assert last["outcome"] == "DONE", rep
    assert t.factors == ml["cycles"] == last["kc"] + last["kt"], (rep, ml)
    assert t.unvisited == ml["unreached"] == last["nu"], (rep, ml)
    assert last["kt"] == ml["unreached_cycles"], (rep, ml)
    assert ml["nu2_lo"] <= last["nu2"] <= ml["nu2_hi"], (rep, ml)
    pred = M.predict(mod, g, mark)
    assert [(a["g"], a["mark"], a["outcome"]) for a in rep] == [(a["g"], a["mark"], a["outcome"]) for a in pred], (rep, pred)
    assert (last["second_collect"], last["unit_rank"]) == (pred[-1]["second_collect"], pred[-1]["unit_rank"]), (rep, pred)
    return pred


SIDE_CELLS = [(4, m) for m in ("moments", "log", "sentinel", "bytemap")] + [(0, "moments"), (6, "moments"), (8, "moments")]


@pytest.mark.parametrize("g,mark", SIDE_CELLS, ids=["g%d-%s" % c for c in SIDE_CELLS])
def test_built_inputs_side_by_side(pkg, g, mark):
    data, lengths, want, mod = built_set("side")
    with fresh_context(pkg, plan="shared", big=ALL, g=g, mark=mark) as ctx:
        got = ctx.inverse_segments(data, lengths)
        t, rep, seg = ctx.timings(), ctx.debug_inverse_report(), ctx.debug_segments_report()
    assert np.array_equal(got, want), (rep, np.flatnonzero(got != want)[:8])
    assert _all_shared(seg, lengths) and seg["attempts"] == len(rep), seg
    pred = check_pass_report(mod, g, mark, rep, t)
    if g > 0:
        # the paths the inputs are there for, all in one pass: the long splitter-free cycles of rot2k-c2odd take the unit-node route,
        # sorted-above alone overfills the first lists, and under the moments the arithmetic gives up (the index log runs the walk again)
        assert rep[-1]["unit_rank"] and rep[-1]["second_collect"], rep
        assert pred[-1]["unit_rank"] and pred[-1]["second_collect"]
    if mark == "moments" and g > 0:
        assert [a["outcome"] for a in rep] == ["NEED_LOG", "DONE"] and rep[1]["mark"] == "log", rep


@pytest.mark.parametrize("mark", ["moments", "bytemap"])
def test_node_pool_overflow_in_a_run(pkg, mark):
    data, lengths, want, mod = built_set("overflow")
    assert mod.at(4)["overflow"]
    with fresh_context(pkg, plan="shared", big=ALL, g=4, mark=mark) as ctx:
        got = ctx.inverse_segments(data, lengths)
        t, rep = ctx.timings(), ctx.debug_inverse_report()
    assert np.array_equal(got, want), (rep, np.flatnonzero(got != want)[:8])
    check_pass_report(mod, 4, mark, rep, t)
    assert [(a["g"], a["outcome"]) for a in rep] == [(4, "RETRY_DENSE"), (0, "DONE")], rep
    assert rep[1]["mark"] == ("bytemap" if mark == "bytemap" else "sentinel"), rep


# ---- the default plan, and plan A as it was ----------------------------------------------------------------------------------------

_big = {}


def zipf_64_segments(seg_len):
    if seg_len not in _big:
        x = O.generate("zipf", 64 * seg_len, 5)
        x.setflags(write=False)
        _big.clear()
        _big[seg_len] = x
    return _big[seg_len], np.full(64, seg_len, dtype=np.uint64)


def test_default_plan_shares_64_segments_of_512k(pkg):
    x, lengths = zipf_64_segments(512 << 10)
    plan = pkg.debug_segments_plan(lengths)
    with fresh_context(pkg) as ctx:
        y = ctx.forward_segments(x, lengths)
        back = ctx.inverse_segments(y, lengths)
        t, rep, chain = ctx.timings(), ctx.debug_segments_report(), ctx.debug_inverse_report()
    assert np.array_equal(back, x)
    assert _all_shared(rep, lengths), rep
    assert {k: rep[k] for k in plan if k != "arena_bytes"} == {k: plan[k] for k in plan if k != "arena_bytes"}, (rep, plan)
    walks = t.k[pkg.K_NAMES.index("walk")].launches
    assert walks == t.attempts == rep["attempts"] == len(chain), (walks, t.attempts, rep, chain)
    assert chain[-1]["form"] == "segmented" and chain[-1]["outcome"] == "DONE"
    assert t.factors == chain[-1]["kc"] + chain[-1]["kt"] and t.n == x.size


def test_default_plan_keeps_tiny_segments_on_the_lane_walk(pkg):
    data, lengths = C.tiny_segments(32, 50000)
    table = C.TinyTable(O.inverse)
    want = table.apply(data, lengths)
    with fresh_context(pkg) as ctx:
        got = ctx.inverse_segments(data, lengths)
        t, rep = ctx.timings(), ctx.debug_segments_report()
    assert np.array_equal(got, want)
    assert rep["plan"] == "lane" and (rep["lane_segments"], rep["lane_bytes"]) == (lengths.size, data.size) and rep["runs"] == 1, rep
    assert (rep["shared_bytes"], rep["single_bytes"]) == (0, 0), rep
    assert t.factors == table.count_factors(want, lengths)


LANE_SEG_LEN = 512 << 10


def test_lane_plan_gives_the_same_bytes(pkg):
    """Plan A pinned as it was: BWTS_SEG_INV_PLAN=lane with every segment below `big` walks each segment on one lane."""
    x, lengths = zipf_64_segments(LANE_SEG_LEN)
    with fresh_context(pkg, plan="shared", big=ALL) as ctx:
        shared = ctx.inverse_segments(x, lengths)
        assert _all_shared(ctx.debug_segments_report(), lengths)
        f_shared = ctx.timings().factors
    with fresh_context(pkg, plan="lane", big=LANE_SEG_LEN + 1) as ctx:
        t0 = time.perf_counter()
        lane = ctx.inverse_segments(x, lengths)
        print("lane walk of 64 x %d bytes: %.2f s" % (LANE_SEG_LEN, time.perf_counter() - t0))
        rep, f_lane = ctx.debug_segments_report(), ctx.timings().factors
    assert rep["plan"] == "lane" and (rep["lane_segments"], rep["lane_bytes"]) == (64, x.size) and rep["single_segments"] == 0, rep
    assert np.array_equal(lane, shared)
    assert f_lane == f_shared
