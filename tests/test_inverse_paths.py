"""GPU suite (-m gpu): every stage and fallback of the inverse, reached with built inputs (tests/inverse_cases.py) and asserted by
name from the engine's own report of what it did (Context.debug_inverse_report) against a CPU model of the walk
(tests/inverse_model.py).  Bytes and counts are exact; nothing here has a tolerance.

Every cell makes a fresh context under BWTS_TEST_KNOBS=1, BWTS_POISON=1 and its own BWTS_SPLIT_LOG2 / BWTS_INV_MARK (a context
reads its knobs when it is made), so the room for unreached elements starts from its default and nothing depends on test order."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import inverse_cases as IC
import inverse_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KNOBS = ("BWTS_TEST_KNOBS", "BWTS_POISON", "BWTS_SPLIT_LOG2", "BWTS_INV_MARK", "BWTS_BYTEMARK", "BWTS_FORCE_WIDE")


@contextlib.contextmanager
def fresh_context(pkg, g=None, mark=None):
    saved = {k: os.environ.get(k) for k in _KNOBS}
    try:
        for k in _KNOBS:
            os.environ.pop(k, None)
        os.environ.update(BWTS_TEST_KNOBS="1", BWTS_POISON="1")
        if g is not None:
            os.environ["BWTS_SPLIT_LOG2"] = str(g)
        if mark is not None:
            os.environ["BWTS_INV_MARK"] = mark
        with pkg.Context(0) as ctx:
            yield ctx
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_prepared = {}


def prepared(case):
    """(B, the oracle's inverse of it, the model) -- kept for the cells of one input, which run one after the other."""
    if case.name not in _prepared:
        _prepared.clear()
        B = np.ascontiguousarray(case.build(), dtype=np.uint8)
        _prepared[case.name] = (B, O.inverse(B), M.Model(B))
    return _prepared[case.name]


_seen = {}           # (case, g, mark) -> the reported chain


def check_report(mod, g, mark, rep, t):
    """(c) the report against the model, (d) the chain of attempts against what the counts decide for a fresh context."""
    assert t.attempts == len(rep) and rep, rep
    for a in rep:
        ma = mod.at(a["g"])
        assert a["form"] == "narrow" and a["s"] == ma["s"] and a["node_cap"] == ma["s"] + ma["room"], (a, ma)
        a["overflow"] = a["outcome"] == "RETRY_DENSE" and a["virtual"] > ma["room"]
        assert a["overflow"] == ma["overflow"], (a, ma)                     # overflow exactly where the model says
        if not ma["overflow"]:
            assert a["virtual"] == ma["virtual"], (a, ma)
    last, ml = rep[-1], mod.at(rep[-1]["g"])
    assert last["outcome"] == "DONE", rep
    assert t.factors == ml["cycles"] == last["kc"] + last["kt"], (rep, ml)
    assert t.unvisited == ml["unreached"] == last["nu"], (rep, ml)
    assert last["kt"] == ml["unreached_cycles"], (rep, ml)
    assert ml["nu2_lo"] <= last["nu2"] <= ml["nu2_hi"], (rep, ml)           # (a range only where virtual node ids decide)
    assert last["ucap_first"] == min(mod.n, M.UNV_CAP0), rep                # a fresh context: no hint from an earlier call
    pred = M.predict(mod, g, mark)
    assert [(a["g"], a["mark"], a["outcome"]) for a in rep] == [(a["g"], a["mark"], a["outcome"]) for a in pred], (rep, pred)
    assert (last["second_collect"], last["unit_rank"]) == (pred[-1]["second_collect"], pred[-1]["unit_rank"]), (rep, pred)
    for a, pa in zip(rep, pred):
        if a["mark"] == "moments" and a["outcome"] != "RETRY_DENSE":        # what the moments made of the unreached elements, by the model's replay
            a["moments"] = pa["moments"]
            assert (a["listed_classes"], a["mom_fallback"] > 0) == (pa["moments"]["listed"], pa["moments"]["fallback"]), (a, pa)
            assert (a["outcome"] == "NEED_LOG") == (a["mom_fallback"] > 0), rep
        else:
            assert a["listed_classes"] == 0 and a["mom_fallback"] == 0, rep


@pytest.mark.parametrize("case,g,mark,home", IC.ALL_CELLS, ids=["%s-g%d-%s" % (c.name, g, m) for c, g, m, _ in IC.ALL_CELLS])
def test_inverse_path(pkg, case, g, mark, home):
    B, want, mod = prepared(case)
    with fresh_context(pkg, g, mark) as ctx:
        got = ctx.inverse(B)
        t, rep = ctx.timings(), ctx.debug_inverse_report()
        back = ctx.forward(got)
    print("%s g=%d %s: %s" % (case.name, g, mark, json.dumps(rep)))
    assert np.array_equal(got, want), (case.name, g, mark, rep, np.flatnonzero(got != want)[:8])      # (a)
    assert np.array_equal(back, B)                                                                      # (b)
    check_report(mod, g, mark, rep, t)                                                                  # (c), the chain of (d)
    if home:                                                                                            # (d) the path this case is there for
        for tag in case.tags:
            assert IC.tag_holds(tag, rep, mark) in (True, None), (tag, rep)
    _seen[(case.name, g, mark)] = rep


def test_attempts_chain_of_the_default_path(pkg):
    """No knob but the gate: g as the engine picks it (4 below 2^28), moments first.  A constant input leaves 15 of 16 elements
    unreached in every class: more than the search's budget, so the index log runs the walk again."""
    z = np.full(6 << 20, 7, dtype=np.uint8)
    with fresh_context(pkg) as ctx:
        assert np.array_equal(ctx.inverse(z), z)
        rep = ctx.debug_inverse_report()
    assert [(a["g"], a["mark"], a["outcome"]) for a in rep] == [(4, "moments", "NEED_LOG"), (4, "log", "DONE")]
    assert rep[0]["mom_fallback"] > 0 and rep[0]["listed_classes"] == 0          # the budget's refusal: it clears the list
    assert rep[1]["nu"] == z.size - z.size // 16 and rep[1]["second_collect"] and not rep[1]["unit_rank"] and rep[1]["kt"] == rep[1]["nu"]


_WIDE = ["rot-c2816-g8", "rot-c2624-g4", "rot2k-c2odd", "rot2k-c32odd", "short-l20-w600", "short-l300-w600", "short-l3-w40", "cycles-r15"]


def test_forced_wide_inverse_same_stages():
    """The 64-bit form (BWTS_FORCE_WIDE=2, splitters every 256 elements) on the rotation and short-factor inputs, in a child process
    as the other forced-wide tests: bytes, and the cycle and unreached counts of the model at g = 8."""
    if os.environ.get("BWTS_TEST_CHILD"):
        pytest.skip("already inside a child run")
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_lib as O, inverse_cases as IC, inverse_model as M, __graft_entry__ as ge
pkg = ge.load_package()
for case in IC.CASES:
    if case.name not in %r: continue
    B = np.ascontiguousarray(case.build(), dtype=np.uint8)
    want, r = O.inverse(B), M.Model(B).at(8)
    with pkg.Context(0) as ctx:
        got = ctx.inverse(B)
        t, rep = ctx.timings(), ctx.debug_inverse_report()
        assert np.array_equal(got, want), (case.name, rep)
        assert (t.factors, t.unvisited) == (r["cycles"], r["unreached"]), (case.name, t.factors, t.unvisited, r, rep)
        assert rep[-1]["form"] == "wide" and rep[-1]["outcome"] == "DONE" and rep[-1]["g"] == 8 and rep[-1]["nu"] == r["unreached"], rep
        if not r["overflow"]: assert rep[-1]["virtual"] == r["virtual"], (rep, r)
    print(case.name, [(a["mark"], a["outcome"], a["virtual"], a["nu"], a["unit_rank"]) for a in rep])
print("wide inverse ok")
""" % (ROOT, os.path.join(ROOT, "tests"), _WIDE)
    env = dict(os.environ, BWTS_TEST_CHILD="1", BWTS_TEST_KNOBS="1", BWTS_FORCE_WIDE="2", BWTS_WIDE_SEG_LOG2="13", BWTS_POISON="1")
    from test_gpu_parity import _wait_gpu_handle_released
    proc = subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT)
    try:
        out, _ = proc.communicate(timeout=900)
    except subprocess.TimeoutExpired:
        proc.kill()
        out, _ = proc.communicate()
    _wait_gpu_handle_released(proc.pid)
    print(out.decode(errors="replace"))
    assert proc.returncode == 0 and b"wide inverse ok" in out, out.decode(errors="replace")[-4000:]


def test_every_path_was_seen():
    """Across the cells above the engine reported every item of the coverage list (tests/inverse_cases.py: COVERAGE) -- the inputs
    are built so that the model alone predicts each (tests/test_inverse_model.py::test_every_path_is_predicted)."""
    assert len(_seen) == len(IC.ALL_CELLS), "this test looks at the reports of the whole file: %d of %d cells ran" % (len(_seen), len(IC.ALL_CELLS))
    seen = set()
    for rep in _seen.values():
        seen |= IC.coverage_of(rep)
    overflowed = [k for k, rep in _seen.items() if rep[0]["outcome"] == "RETRY_DENSE" and rep[0]["overflow"]]
    assert overflowed, "RETRY_DENSE by node-pool overflow"
    assert not [c for c in IC.COVERAGE if c not in seen], sorted(seen)
