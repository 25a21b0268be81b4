"""GPU suite (-m gpu): every stage of the forward's sort, reached with built inputs (tests/forward_cases.py) and asserted by name
from the engine's own report of what it did (Context.debug_forward_report) against a numpy model of the rounds
(tests/forward_model.py).  Bytes and counts are exact; nothing here has a tolerance.

Every cell makes a fresh context under BWTS_TEST_KNOBS=1 BWTS_POISON=1 and its own knobs (a context reads them when it is made)."""
import contextlib
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import forward_cases as FC
import forward_model as M
import key_model as KM
import oracle_lib as O

pytestmark = pytest.mark.gpu

_KNOBS = ("BWTS_TEST_KNOBS", "BWTS_POISON", "BWTS_VARLEN", "BWTS_KEY_SYMBOLS", "BWTS_KEY_BITS", "BWTS_DENSE", "BWTS_BIGLIST_NOMEM", "BWTS_RX_PACK",
          "BWTS_EMIT", "BWTS_LYNDON", "BWTS_ROUND_TRACE", "BWTS_FORCE_WIDE", "BWTS_CHUNK_TARGET")


@contextlib.contextmanager
def fresh_context(pkg, env):
    saved = {k: os.environ.get(k) for k in _KNOBS}
    try:
        for k in _KNOBS:
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


def chunk_plan(pkg):
    def plan(a0, a_chunks, target=M.CHUNK_TARGET):
        out = (ctypes.c_uint64 * 4)()
        fits = pkg.lib().bwts_debug_chunk_plan_target(a0, a_chunks, target, out)
        assert fits in (0, 1)
        return [int(v) for v in out], bool(fits)
    return plan


_prepared = {}


def prepared(case):
    """(x, the oracle's transform, the cyclic model, the suffix model) of the input, kept while consecutive cells use the same one."""
    x = np.ascontiguousarray(case.build(), dtype=np.uint8)
    key = hashlib.sha256(x.tobytes()).digest()
    if _prepared.get("key") != key:
        _prepared.clear()
        _prepared.update(key=key, x=x, want=O.forward(x), cyclic=M.Model(x), suffix=None)
    if case.sort != "cyclic" and _prepared["suffix"] is None:
        _prepared["suffix"] = M.Model(x, cyclic=False)
    return _prepared


_seen = {}


def check_exact(rep, p, t=None):
    """The report of one sort against the prediction for fixed-width keys: every header word and every round, exactly."""
    for f in ("cyclic", "n", "k", "sigma", "bits", "msym", "key_bits", "varlen", "hstep", "keys", "flags_outside_rank", "tied0", "rank_early",
              "form", "no_chunks", "need_sa", "end", "rounds", "left"):
        assert rep[f] == p[f], (f, rep[f], p[f])
    if p["form"] == "sparse":
        assert rep["directory"] == p["directory"], (rep["directory"], p["directory"])
    if p["form"] == "tiles":
        assert (rep["order_sort"], rep["rest_tiles"], rep["rest_chunks"], rep["rest_big"]) == (p["order_sort"], p["rest_tiles"], 0, 0), rep
    if p["form"] == "chunks":
        assert rep["chunks"] == p["chunks"], (rep["chunks"], p["chunks"])
        assert (rep["chunk_S_recut"], rep["chunk_round_S"]) == (p["chunk_S_recut"], p["chunk_round_S"]), (rep["chunk_S_recut"], rep["chunk_round_S"])
        assert (rep["rest_chunks"], rep["rest_big"], rep["rest_tiles"]) == (p["rest_chunks"], p["rest_big"], 0), rep
    assert len(rep["round"]) == len(p["round"]) == rep["rounds"] - 1
    for r, pr in zip(rep["round"], p["round"]):
        # (the engine's word is a flag, 1 once any group of the round split: exactly "the classes grew")
        assert r["splits"] == int(pr["split"]), (r, pr)
        assert {k: v for k, v in r.items() if k != "splits"} == {k: v for k, v in pr.items() if k != "split"}, (r, pr)
    # tied after every round: the report's own account and the model's (the engine may never split a group later, nor earlier)
    assert [rep["tied0"]] + [r["out"] for r in rep["round"]] == p["round_active"]
    if t is not None:                                                   # bwts_timings tells the same story (cyclic sort only)
        assert t.rounds == p["rounds"] and t.active_after_round0 == p["tied0"] and t.factors == p["k"]
        assert [int(v) for v in t.round_active[:t.rounds]] == p["round_active"], ([int(v) for v in t.round_active[:t.rounds]], p["round_active"])


def check_any_key(rep, mod, t, pkg):
    """No key knob: the heuristics pick the key.  Fixed-width keys are still exact (the caller does that).  For variable-length keys
    the model builds every position's key from the code table of the input's histogram (debug_key_plan: csrc/key_plan.h) at the
    width the engine reports (from 2^22 positions on its key sample may have widened it) and the tied count after round 0 is exact
    too (tests/key_model.py); the rest is what holds for any key whose first step is hstep symbols."""
    final = mod.final_tied()
    if rep["varlen"]:
        plan = pkg.debug_key_plan(np.bincount(mod.x, minlength=256), varlen=1, key_bits=rep["key_bits"])
        assert (plan["key_bits"], plan["hstep"], plan["msym"], plan["bits"]) == (rep["key_bits"], rep["hstep"], rep["msym"], rep["bits"]), rep
        assert rep["hstep"] == max(1, rep["key_bits"] // plan["lmax"])
        assert rep["tied0"] == KM.tied(KM.keys_of_plan(mod.x, mod.starts, plan)), rep["tied0"]
    assert mod.stats(rep["hstep"])["tied"] >= rep["tied0"] >= final, (rep["tied0"], final)
    active = [int(v) for v in t.round_active[:t.rounds]]
    assert active == [rep["tied0"]] + [r["out"] for r in rep["round"]] and t.rounds == rep["rounds"]
    assert all(a >= b for a, b in zip(active, active[1:])), active
    assert active[-1] == rep["left"] == (final if rep["end"] != "none" or rep["tied0"] else 0), (active, final)
    assert rep["end"] == ("none" if rep["tied0"] == 0 else "stable" if final else "empty")
    assert rep["rest_chunks"] + rep["rest_big"] + rep["rest_tiles"] == (final if rep["form"] in ("chunks", "tiles") else 0)


@pytest.mark.parametrize("case", FC.CASES, ids=[c.name for c in FC.CASES])
def test_forward_path(pkg, case):
    pre = prepared(case)
    x, want = pre["x"], pre["want"]
    env = dict(case.env, BWTS_VARLEN="0", BWTS_KEY_SYMBOLS=str(case.m))
    if case.sort == "general":
        env["BWTS_LYNDON"] = "general"
    knobs = dict(tiles_knob=env.get("BWTS_DENSE") == "tiles", biglist_nomem="BWTS_BIGLIST_NOMEM" in env, gather=env.get("BWTS_EMIT") == "gather",
                 pack=env.get("BWTS_RX_PACK") != "0", target=int(env.get("BWTS_CHUNK_TARGET", M.CHUNK_TARGET)))
    with fresh_context(pkg, env) as ctx:
        if case.sort == "suffix":
            sa = ctx.debug_suffix_array(x)
            reps, t = ctx.debug_forward_report(), None
        else:
            got = ctx.forward(x)
            t, reps = ctx.timings(), ctx.debug_forward_report()
            back = ctx.inverse(got)
    print("%s: %s" % (case.name, json.dumps(reps)))
    plan = chunk_plan(pkg)
    if case.sort == "suffix":
        assert np.array_equal(sa.astype(np.int64), O.suffix_array(x).astype(np.int64))
        assert len(reps) == 1
        check_exact(reps[0], M.predict(pre["suffix"], case.m, plan, **knobs))
        home = reps[0]
    else:
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert np.array_equal(back, x)
        # (a forward that found its factors by the suffix route -- asked for, or picked for an input of many equal factors -- reports
        # that sort first)
        assert len(reps) in ((2,) if case.sort == "general" else (1, 2)) and reps[-1]["cyclic"] and not any(r["cyclic"] for r in reps[:-1]), reps
        check_exact(reps[-1], M.predict(pre["cyclic"], case.m, plan, **knobs), t)
        home = reps[-1]
        if case.sort == "general":                  # the suffix sort first; both sorts see the same key knob
            check_exact(reps[0], M.predict(pre["suffix"], case.m, plan, tiles_knob=knobs["tiles_knob"], biglist_nomem=knobs["biglist_nomem"],
                                              target=knobs["target"]))
            home = reps[0]
    for tag in case.tags:
        assert FC.tag_holds(tag, home), (tag, home)
    _seen[case.name] = home


@pytest.mark.parametrize("case", FC.DEFAULT_KEY_CASES, ids=[c.name for c in FC.DEFAULT_KEY_CASES])
def test_forward_default_key(pkg, case):
    pre = prepared(case)
    x, want, mod = pre["x"], pre["want"], pre["cyclic"]
    with fresh_context(pkg, {}) as ctx:
        got = ctx.forward(x)
        t, reps = ctx.timings(), ctx.debug_forward_report()
        back = ctx.inverse(got)
    print("%s (default key): %s" % (case.name, json.dumps(reps)))
    assert np.array_equal(got, want) and np.array_equal(back, x)
    assert len(reps) in (1, 2) and reps[-1]["cyclic"] and not any(r["cyclic"] for r in reps[:-1]), reps
    rep = reps[-1]
    assert t.key_bits == rep["key_bits"] and t.key_symbols == rep["msym"]
    check_any_key(rep, mod, t, pkg)
    if not rep["varlen"]:
        check_exact(rep, M.predict(mod, rep["msym"], chunk_plan(pkg)), t)
    _seen[case.name + "/default"] = rep


def test_every_path_was_seen():
    """Across the cells above the engine reported every name of the coverage list (the inputs are built so that the model alone
    predicts each: tests/test_forward_model.py::test_every_path_is_predicted)."""
    assert len([k for k in _seen if "/" not in k]) == len(FC.CASES), "this test looks at the reports of the whole file"
    seen = {}
    for c in FC.CASES:
        for tag in FC.COVERAGE:
            try:
                if tag not in seen and FC.tag_holds(tag, _seen[c.name]):
                    seen[tag] = c.name
            except KeyError:
                pass
    print(json.dumps(seen, indent=1, sort_keys=True))
    assert not [t for t in FC.COVERAGE if t not in seen], sorted(seen)
