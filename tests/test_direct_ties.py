"""GPU suite (-m gpu): the direct form of the forward's later rounds (direct_ties_kernel: every tied group ordered by one thread that
compares its members' rotations), reached below its default size gate with BWTS_DIRECT_MIN_LOG2=0.

Every case compares the device's bytes with the oracle's exactly AND asserts header word 36 of the engine's report (0 not tried,
1 all groups settled, 2 fell back on a group above the cap, 3 fell back on depth): a case meant for the direct form must report 1,
so a silent fallback cannot make it pass.  The stated property of every input (tied count <= n / 32, group sizes, period sums) is
asserted from the numpy model of the rounds (tests/forward_model.py) next to the device run.  The cells fix the key
(BWTS_VARLEN=0 BWTS_KEY_SYMBOLS=m) so that those properties hold by construction, not by what the key heuristics pick."""
import contextlib
import json
import os

import numpy as np
import pytest

import forward_cases as FC
import forward_model as M
import oracle_lib as O
from test_forward_paths import _KNOBS, check_exact, chunk_plan

pytestmark = pytest.mark.gpu

DIRECT_GROUP = 8          # csrc/forward.hip: members one thread orders
DIRECT_DEPTH = 640        # ... symbols it compares before it gives a pair up
NOT_TRIED, SETTLED, FELL_BACK_GROUP, FELL_BACK_DEPTH = 0, 1, 2, 3


@contextlib.contextmanager
def fresh_context(pkg, env):
    """A context made under BWTS_TEST_KNOBS=1 BWTS_POISON=1 and `env` alone; the environment is put back afterwards."""
    names = set(_KNOBS) | {"BWTS_DIRECT_MIN_LOG2"} | set(env)
    saved = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(BWTS_TEST_KNOBS="1", BWTS_POISON="1", **env)
        with pkg.Context(0) as ctx:
            yield ctx
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(pkg, x, m, env=None, gate="0"):
    """One forward on a fresh context: (bytes, timings, reports).  gate None: no BWTS_DIRECT_MIN_LOG2 (the default gate)."""
    e = {"BWTS_VARLEN": "0", "BWTS_KEY_SYMBOLS": str(m)} if m else {}
    if gate is not None:
        e["BWTS_DIRECT_MIN_LOG2"] = gate
    e.update(env or {})
    with fresh_context(pkg, e) as ctx:
        got = ctx.forward(x)
        t, reps = ctx.timings(), ctx.debug_forward_report()
    print(json.dumps(reps))
    return got, t, reps


def tied_groups(mod, m):
    """(tied positions, sizes of the tied groups) after a round 0 of m symbols."""
    cnt = np.bincount(mod.classes(m))
    return int(cnt[cnt > 1].sum()), cnt[cnt > 1]


def assert_direct(rep, t, tied):
    """The report of a sort that the direct form settled: one round after round 0, nothing left."""
    assert rep["cyclic"] and rep["direct_word"] == SETTLED and rep["form"] == "direct", rep
    assert rep["tied0"] == tied and rep["rounds"] == 2 and rep["left"] == 0 and rep["end"] == "empty", rep
    assert rep["round"] == [{"form": "direct", "h": rep["hstep"], "in": tied, "out": 0, "splits": 1}], rep["round"]
    assert t.rounds == 2 and [int(v) for v in t.round_active[:2]] == [tied, 0]


def assert_sparse_as_before(pkg, rep, t, mod, m, **knobs):
    """The sparse form, word for word what the model of the rounds predicts (as tests/test_forward_paths.py pins it)."""
    assert rep["form"] == "sparse", rep
    check_exact(rep, M.predict(mod, m, chunk_plan(pkg), **knobs), t)


def wrapped_pairs(blocks, length, seed):
    """Like forward_cases.many_factors_twice, but the first word of every pair has its second letter raised by one: Lyndon words w' > w
    with falling first letters.  Rotations of w' and w at the same offset behind that letter agree until they have run round the
    factor's end and reach it again: the comparison is decided after the wrap."""
    rng = np.random.default_rng(seed)
    parts = []
    for c in range(blocks - 1, -1, -1):
        w = np.concatenate([[3 * c], rng.integers(3 * c + 1, 3 * c + 40, length - 1)]).astype(np.uint8)
        w2 = w.copy()
        w2[1] += 1
        parts += [w2, w]
    return np.concatenate(parts)


def above(head_n, tail, seed):
    """Noise over letters above every letter of `tail`, then `tail`: the factors are the noise's own, then the tail's."""
    base = int(tail.max()) + 1
    assert base < 200
    return np.concatenate([FC.noise(head_n, 256 - base, seed, base=base), tail])


SMALL_GROUPS = [
    ("noise4-seed2", lambda: FC.noise(1 << 18, 4, 2), 12, 2000, 3),
    ("noise4-seed3", lambda: FC.noise(1 << 18, 4, 3), 12, 1900, 3),
    # a phrase with four different tails, eight times in all: groups of 8 that come apart into pairs 18 .. 47 symbols on
    ("variants-8", lambda: FC.variants(1 << 18, 4, 5, 30, 30, 4, 8), 12, 2000, 8),
]


@pytest.mark.parametrize("name,build,m,min_groups,largest", SMALL_GROUPS, ids=[c[0] for c in SMALL_GROUPS])
def test_pairs_and_small_groups(pkg, name, build, m, min_groups, largest):
    """Noise over 4 letters, keys of 12 symbols: a few thousand tied positions, nearly all in pairs, some groups of 3 and more."""
    x = build()
    mod = M.Model(x)
    tied, sizes = tied_groups(mod, m)
    assert min_groups <= sizes.size and tied <= x.size // 32 and sizes.max() == largest <= DIRECT_GROUP, (tied, np.bincount(sizes))
    got, t, reps = run(pkg, x, m)
    assert np.array_equal(got, O.forward(x))
    assert len(reps) == 1
    assert_direct(reps[0], t, tied)


def test_group_above_the_cap(pkg):
    """200 copies of a phrase: groups of 200.  The kernel raises its flag and the sparse rounds run as they always did."""
    x, m = FC.pasted(1 << 20, 4, 5, [(40, 200)]), 13
    mod = M.Model(x)
    tied, sizes = tied_groups(mod, m)
    assert tied <= x.size // 32 and sizes.max() > DIRECT_GROUP
    got, t, reps = run(pkg, x, m)
    assert np.array_equal(got, O.forward(x))
    assert reps[-1]["direct_word"] == FELL_BACK_GROUP, reps[-1]
    assert_sparse_as_before(pkg, reps[-1], t, mod, m)


SHORT_PERIODS = [
    ("equal-factors-300", lambda: FC.equal_factors_in_noise(1 << 17, 300, 7), 4, 300),
    # a Lyndon word of 100 letters eight times over: groups of 8 equal rotations, the cap itself
    ("factor-100-x8", lambda: FC.factor_many_times(100, DIRECT_GROUP, 1 << 16, 9), 5, 100),
]


@pytest.mark.parametrize("name,build,m,period", SHORT_PERIODS, ids=[c[0] for c in SHORT_PERIODS])
def test_equal_rotations_short_period(pkg, name, build, m, period):
    """Equal factors whose lengths sum to less than DIRECT_DEPTH: rotations that agree on that many symbols are equal for ever
    (Fine and Wilf), emit the same byte and count as settled."""
    x = build()
    mod = M.Model(x)
    tied, sizes = tied_groups(mod, m)
    lens = np.diff(np.append(mod.starts, x.size))
    assert tied <= x.size // 32 and sizes.max() <= DIRECT_GROUP and mod.final_tied(m) >= 2 * period and 2 * period < DIRECT_DEPTH
    assert (lens == period).sum() >= 2
    got, t, reps = run(pkg, x, m)
    assert np.array_equal(got, O.forward(x))
    assert_direct(reps[-1], t, tied)


LONG_PERIODS = [
    ("equal-factors-321", lambda: FC.equal_factors_in_noise(1 << 17, 321, 7), 4, 321),     # 642: just above the depth
    ("equal-factors-1500", lambda: FC.equal_factors_in_noise(1 << 17, 1500, 7), 4, 1500),
    ("factor-700-x2", lambda: FC.factor_many_times(700, 2, 1 << 16, 9), 5, 700),
]


@pytest.mark.parametrize("name,build,m,period", LONG_PERIODS, ids=[c[0] for c in LONG_PERIODS])
def test_equal_rotations_long_period(pkg, name, build, m, period):
    """Equal factors whose lengths sum to more than DIRECT_DEPTH: undecided at the depth, so the sparse rounds run and end, as they
    did, on a round that splits no group."""
    x = build()
    mod = M.Model(x)
    tied, sizes = tied_groups(mod, m)
    assert tied <= x.size // 32 and sizes.max() <= DIRECT_GROUP and 2 * period > DIRECT_DEPTH
    got, t, reps = run(pkg, x, m)
    assert np.array_equal(got, O.forward(x))
    assert reps[-1]["direct_word"] == FELL_BACK_DEPTH, reps[-1]
    assert_sparse_as_before(pkg, reps[-1], t, mod, m)
    assert reps[-1]["end"] == "stable" and reps[-1]["left"] == 2 * period


WRAPS = [
    # every position of the pairs is tied for ever, the 60 factor heads included (their byte is the factor's last one)
    ("twice-20", lambda: above(1 << 17, FC.many_factors_twice(30, 20, 10), 11), 5, True),
    ("twice-7", lambda: above(1 << 17, FC.many_factors_twice(30, 7, 12), 13), 5, True),
    # pairs that differ in one early letter: decided only after the window has run round the factor
    ("wrapped-pairs-20", lambda: above(1 << 17, wrapped_pairs(30, 20, 14), 15), 5, False),
    ("wrapped-pairs-9", lambda: above(1 << 17, wrapped_pairs(30, 9, 16), 17), 5, False),
]


@pytest.mark.parametrize("name,build,m,equal", WRAPS, ids=[c[0] for c in WRAPS])
def test_wrap_inside_the_window(pkg, name, build, m, equal):
    """Factors shorter than hstep + 64: the compared windows run round their factor, more than once for the equal pairs."""
    x = build()
    mod = M.Model(x)
    tied, sizes = tied_groups(mod, m)
    lens = np.diff(np.append(mod.starts, x.size))
    cls = mod.classes(m)
    head_tied = (np.bincount(cls)[cls[mod.starts]] > 1)
    assert tied <= x.size // 32 and sizes.max() <= DIRECT_GROUP and tied >= 200, (tied, sizes.max())
    assert (lens < m + 64).sum() >= 60 and mod.final_tied(m) == (tied if equal else 0)
    assert (lens[head_tied] < m + 64).sum() == (60 if equal else 0), "tied heads of short factors"
    got, t, reps = run(pkg, x, m)
    assert np.array_equal(got, O.forward(x))
    assert_direct(reps[-1], t, tied)


@pytest.mark.parametrize("n,form", [(1 << 24, "direct"), ((1 << 24) - 1, "sparse")])
def test_default_gate(pkg, n, form):
    """No BWTS_DIRECT_MIN_LOG2 and no key knob: the direct form is the default from 2^24 positions and not tried below."""
    x = FC.noise(n, 4, 21)
    got, t, reps = run(pkg, x, None, gate=None)
    assert np.array_equal(got, O.forward(x))
    rep = reps[-1]
    assert 0 < rep["tied0"] <= n // 32, rep
    assert rep["form"] == form and rep["direct_word"] == (SETTLED if form == "direct" else NOT_TRIED), rep
    if form == "direct":
        assert_direct(rep, t, rep["tied0"])


def test_gate_knob_turns_it_off(pkg):
    """BWTS_DIRECT_MIN_LOG2=64: never tried (the switch of a before/after measurement inside one build)."""
    x, m = FC.noise(1 << 18, 4, 2), 12
    got, t, reps = run(pkg, x, m, gate="64")
    assert np.array_equal(got, O.forward(x))
    assert reps[-1]["direct_word"] == NOT_TRIED
    assert_sparse_as_before(pkg, reps[-1], t, M.Model(x), m)


def test_not_taken_gather(pkg):
    """BWTS_EMIT=gather: no byte rode round 0, the emission reads the whole suffix array, so the rounds must leave it sorted."""
    x, m = FC.noise(1 << 18, 4, 2), 12
    got, t, reps = run(pkg, x, m, env={"BWTS_EMIT": "gather"})
    assert np.array_equal(got, O.forward(x))
    assert reps[-1]["direct_word"] == NOT_TRIED
    assert_sparse_as_before(pkg, reps[-1], t, M.Model(x), m, gather=True)


def test_not_taken_two_segments(pkg):
    """Two segments in one pass: the partition by segment reads the suffix array as well."""
    a, b, m = FC.noise(1 << 17, 4, 31), FC.noise((1 << 17) + 5, 4, 32), 12
    x = np.concatenate([a, b])
    with fresh_context(pkg, {"BWTS_VARLEN": "0", "BWTS_KEY_SYMBOLS": str(m), "BWTS_DIRECT_MIN_LOG2": "0"}) as ctx:
        got = ctx.forward_segments(x, [a.size, b.size])
        reps = ctx.debug_forward_report()
    print(json.dumps(reps))
    assert np.array_equal(got, np.concatenate([O.forward(a), O.forward(b)]))
    assert reps[-1]["cyclic"] and 0 < reps[-1]["tied0"] <= x.size // 32 and reps[-1]["form"] == "sparse", reps[-1]
    assert reps[-1]["direct_word"] == NOT_TRIED


def test_not_taken_suffix_sort(pkg):
    """BWTS_LYNDON=general: the suffix sort that finds the factors has few ties too, and it is not a cyclic sort -- suffixes have no
    factor to run round and the sort's ranks are read afterwards.  It reports 0 and the sparse form; the cyclic sort behind it works on
    the factors that sort found, so the exact bytes also check them."""
    x, m = FC.noise(1 << 18, 4, 2), 12
    got, t, reps = run(pkg, x, m, env={"BWTS_LYNDON": "general"})
    assert np.array_equal(got, O.forward(x))
    assert len(reps) == 2 and not reps[0]["cyclic"] and reps[1]["cyclic"]
    assert 0 < reps[0]["tied0"] <= x.size // 32 and reps[0]["form"] == "sparse" and reps[0]["direct_word"] == NOT_TRIED, reps[0]
    check_exact(reps[0], M.predict(M.Model(x, cyclic=False), m, chunk_plan(pkg)))
