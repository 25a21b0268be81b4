"""CPU suite: the model of the forward's rounds (tests/forward_model.py) against brute force, hand-worked cases and the oracle, and
the coverage list of tests/forward_cases.py against the model's prediction."""
import ctypes

import numpy as np
import pytest

import forward_cases as FC
import forward_model as M
import oracle_lib as O


def chunk_plan(pkg):
    def plan(a0, a_chunks, target=M.CHUNK_TARGET):
        out = (ctypes.c_uint64 * 4)()
        fits = pkg.lib().bwts_debug_chunk_plan_target(a0, a_chunks, target, out)
        assert fits in (0, 1)
        return [int(v) for v in out], bool(fits)
    return plan


def _small_inputs():
    rng = np.random.default_rng(3)
    fib = [b"a", b"ab"]
    while len(fib[-1]) < 200:
        fib.append(fib[-1] + fib[-2])
    yield "fibonacci", np.frombuffer(fib[-1], dtype=np.uint8)
    yield "periodic", np.frombuffer(b"abcab" * 30 + b"abd", dtype=np.uint8)
    yield "many-factors", np.frombuffer(b"zyxwvuttsrqponm" + b"ba" * 20 + b"a" * 7, dtype=np.uint8)
    for i in range(4):
        yield "random-%d" % i, rng.integers(0, [2, 3, 4, 200][i], size=int(rng.integers(40, 160)), dtype=np.uint8)


SMALL = list(_small_inputs())


@pytest.mark.parametrize("name,x", SMALL, ids=[n for n, _ in SMALL])
def test_factor_starts_by_brute_force(name, x):
    assert list(O.lyndon_starts(x)) == M.brute_lyndon_starts(x)


@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("name,x", SMALL, ids=[n for n, _ in SMALL])
def test_classes_against_written_out_words(name, x, cyclic):
    mod = M.Model(x, cyclic)
    starts = M.brute_lyndon_starts(x)
    for d in (1, 2, 3, 5, 8, 12, 16, 48, 64, 3 * len(x)):
        assert np.array_equal(mod.classes(d), M.brute_classes(x, starts, d, cyclic) + (0 if cyclic else 1)), (name, d)
    if not cyclic:
        assert mod.stats(len(x))["tied"] == 0                           # suffixes are distinct


@pytest.mark.parametrize("name,x", SMALL, ids=[n for n, _ in SMALL])
def test_final_order_is_the_transform(name, x):
    """Rotations sorted by brute force, the classes' order and the oracle agree."""
    mod = M.Model(x)
    assert np.array_equal(mod.transform(), O.forward(x)), name
    starts = M.brute_lyndon_starts(x)
    deep = M.brute_classes(x, starts, 2 * len(x) + 2, True)
    assert mod.final_tied() == int((np.bincount(deep)[deep] > 1).sum())


def test_hand_worked_cases():
    # "abab": one... no: factors ab, ab.  Positions 0, 2 read (ab)^inf, positions 1, 3 read (ba)^inf: two groups of two, for ever
    mod = M.Model(np.frombuffer(b"abab", dtype=np.uint8))
    assert list(mod.starts) == [0, 2]
    st, end = mod.walk(1, 2)
    assert [s["tied"] for s in st] == [4, 4] and end == "stable" and list(mod.classes(64)) == [0, 1, 0, 1]
    # "banana": factors b, an, an, a.  Infinite words: b^inf; (an)^inf twice; (na)^inf twice; a^inf.  One symbol ties a with both an
    # (3 in a group) and the two na; two symbols separate a (aa) from an: 4 tied, and they stay
    mod = M.Model(np.frombuffer(b"banana", dtype=np.uint8))
    assert list(mod.starts) == [0, 1, 3, 5]
    st, end = mod.walk(1, 2)
    assert [s["tied"] for s in st] == [5, 4, 4] and end == "stable"
    assert [s["tied"] for s in mod.walk(1, 4)[0]] == [5, 4, 4]
    assert bytes(mod.transform()) == bytes(O.forward(b"banana"))
    # suffix form of "banana": a, ana, anana share "a"; na, nana share "n": 5 tied at depth 1; ana / anana and na / nana at depth 2 and 3;
    # at depth 4 "ana$" and "anan" differ, "na$" and "nan" differed at 3 already
    mod = M.Model(np.frombuffer(b"banana", dtype=np.uint8), cyclic=False)
    assert [mod.stats(d)["tied"] for d in (1, 2, 3, 4)] == [5, 4, 2, 0]
    assert [s["tied"] for s in mod.walk(1, 2)[0]] == [5, 4, 0] and [s["tied"] for s in mod.walk(1, 4)[0]] == [5, 0]
    # group sizes against the thresholds: 3000 copies of a factor of 30
    mod = M.Model(FC.factor_many_times(30, 3000, 500, 1))
    s = mod.walk(4, 4)[0][-1]
    assert (s["tied"], s["huge"], s["huge_groups"], s["le_cap"], s["mid"]) == (90000, 90000, 30, 0, 0)


_pred = {}


def prediction(case, plan):
    if case.name not in _pred:
        mod = M.Model(case.build(), cyclic=case.sort != "suffix")
        if case.sort == "general":
            mod = M.Model(mod.x, cyclic=False)
        _pred[case.name] = M.predict(mod, case.m, plan, tiles_knob=case.env.get("BWTS_DENSE") == "tiles", biglist_nomem="BWTS_BIGLIST_NOMEM" in case.env,
                                     gather=case.env.get("BWTS_EMIT") == "gather", pack=case.env.get("BWTS_RX_PACK") != "0", target=int(case.env.get("BWTS_CHUNK_TARGET", M.CHUNK_TARGET)))
    return _pred[case.name]


@pytest.mark.parametrize("case", FC.CASES, ids=[c.name for c in FC.CASES])
def test_case_is_predicted_to_take_its_paths(pkg, case):
    p = prediction(case, chunk_plan(pkg))
    for tag in case.tags:
        assert FC.tag_holds(tag, p), (tag, {k: v for k, v in p.items() if k != "round"}, p["round"])


def test_every_path_is_predicted(pkg):
    plan = chunk_plan(pkg)
    seen = {t for c in FC.CASES for t in c.tags if FC.tag_holds(t, prediction(c, plan))}
    assert not [t for t in FC.COVERAGE if t not in seen]
    assert FC.NOT_REACHABLE == []
