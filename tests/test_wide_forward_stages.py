"""The forward beyond 2^32 positions (wide_path.h), forced onto small inputs: every stage of a run, every mode and every hand-over
between runs, checked twice over -- the bytes against the oracle, and what each call DID against what the commit before the
host-side restructuring did (tests/golden/wide_forward_stages_parent.json, recorded by running CHILD below against a build of that
commit): the rounds, the factor and key figures, and for every kernel class the launches, elements and algorithmic bytes that the
SpanGuards count on the host.  Those are equal exactly when the same stages ran in the same sequence over the same sizes, runs that
ended in "run again with the rank array / with the suffix route" included.  Times and device_bytes are not compared.

The arena is poisoned (BWTS_POISON=1): an array the layout placed wrongly, or left out, reads as wrong bytes.

Cases (segments of 2^13 positions throughout):
  a  zipf 70001 seed 3, bucket n/6                       direct form, sample taken (n mod 2^13 >= 4096), finishes
  b  text 204000 seed 7, bucket n/6                      direct -> "needs ranks" at the sample -> ranks: more radix passes than the ranks run
     alone makes (b_ranks: the same with direct 0)
  c  text 300007 seed 11, bucket n/5, part 3000, tblock 2^12, direct 0      dozens of parts per round, the list across blocks
  d  dna 200003 seed 13, bucket n/5, part 64, tblock 2^8, direct 0          the smallest parts
  e  dna 400003 seed 22, bucket n/7, direct 1            direct groups forced
  f  text 200003 seed 25, bucket n/6, direct 1           refused with BWTS_E_RANGE (-5); what ran until then is compared too
  g  Lyndon blocks (about 2^18 bytes), lyndon auto, bucket n/2, part n/2    candidates overflow -> suffix route -> cyclic run
  h  case a's input, lyndon suffix                       suffix route first
  i  a descending sorted run of 10^4 bytes, rotated, bucket 4096            thousands of one-symbol factors in the patch and head kernels
  j  b"mississippi", bucket 256                          n far below every capacity
  k  a then b in ONE context (bucket of b)               arena laid out anew per run, tied blocks carried over
  p  a period of 10^5 bytes (its first byte the smallest, once) three times, the last copy broken 7 * 10^4 bytes in: the candidate at
     the second copy agrees with the first for 1.7 * 10^5 bytes, so the resolver hands the comparison to the grid-wide kernel.  Run on
     the wide path, and -- BWTS_FORCE_WIDE unset for that context -- on the narrow path: both callers of the shared resolver.

Every case reached the route named here on the commit before (checked once with prints in a scratch build of it: a 4465 keys sampled, no
tie; b 416 ties in 7392 sampled keys; c 78 parts in the first round, 57 list blocks; g 69 670 candidates; p two grid-wide
comparisons on either path)."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_parity import _child_report, _wait_gpu_handle_released

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
FIXTURE = os.path.join(TESTS, "golden", "wide_forward_stages_parent.json")
ENV = {"BWTS_TEST_KNOBS": "1", "BWTS_FORCE_WIDE": "2", "BWTS_WIDE_SEG_LOG2": "13", "BWTS_POISON": "1"}
KNOBS = ("BWTS_WIDE_LYNDON", "BWTS_WIDE_BUCKET", "BWTS_WIDE_PART", "BWTS_WIDE_DIRECT", "BWTS_WIDE_TBLOCK_LOG2", "BWTS_WIDE_CARRY")

CHILD = r"""
import json, os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_lib as O, lyndon_blocks as LB, __graft_entry__ as ge
pkg = ge.load_package()
KNOBS = %r

def figures(ctx):
    t = ctx.timings()
    return {"rounds": int(t.rounds), "lyndon_rounds": int(t.lyndon_rounds), "factors": int(t.factors), "key_symbols": int(t.key_symbols),
            "key_bits": int(t.key_bits), "active_after_round0": int(t.active_after_round0),
            "round_active": [int(v) for v in t.round_active[:int(t.rounds)]],
            "k": {pkg.K_NAMES[c]: [int(t.k[c].launches), int(t.k[c].elems), int(t.k[c].alg_bytes)] for c in range(pkg.K_COUNT)}}

def context(knobs, wide=True):
    # a context reads its knobs when it is made
    for k in KNOBS: os.environ.pop(k, None)
    os.environ.update({"BWTS_WIDE_" + k.upper(): str(v) for k, v in knobs.items()})
    forced = os.environ.pop("BWTS_FORCE_WIDE") if not wide else None
    try:
        return pkg.Context(0)
    finally:
        if forced is not None: os.environ["BWTS_FORCE_WIDE"] = forced

def forward(ctx, x, refused=False):
    try:
        y = ctx.forward(x)
    except pkg.BwtsError as e:
        assert refused and e.code == -5, e
        return figures(ctx)
    assert not refused, "the forced direct form took an input it must refuse"
    assert np.array_equal(y, O.forward(x))
    return figures(ctx)

def case(x, refused=False, wide=True, **knobs):
    with context(knobs, wide) as ctx:
        return forward(ctx, x, refused)

out = {}
xa, xb = O.generate("zipf", 70001, 3), O.generate("text", 204000, 7)
out["a"] = case(xa, bucket=xa.size // 6)
out["b"] = case(xb, bucket=xb.size // 6)
out["b_ranks"] = case(xb, bucket=xb.size // 6, direct=0)
x = O.generate("text", 300007, 11)
out["c"] = case(x, bucket=x.size // 5, part=3000, tblock_log2=12, direct=0)
x = O.generate("dna", 200003, 13)
out["d"] = case(x, bucket=x.size // 5, part=64, tblock_log2=8, direct=0)
x = O.generate("dna", 400003, 22)
out["e"] = case(x, bucket=x.size // 7, direct=1)
x = O.generate("text", 200003, 25)
out["f"] = case(x, refused=True, bucket=x.size // 6, direct=1)
x, _ = LB.lyndon_blocks(2000, 17 + np.arange(2000) // 30, 20, 200, 1)
out["g"] = case(x, lyndon="auto", bucket=x.size // 2, part=x.size // 2)
out["h"] = case(xa, lyndon="suffix", bucket=xa.size // 6)
x = np.roll(np.sort(np.random.default_rng(3).integers(0, 256, 10000).astype(np.uint8))[::-1], 3333).copy()
out["i"] = case(x, bucket=4096)
out["j"] = case(np.frombuffer(b"mississippi", np.uint8).copy(), bucket=256)
with context({"bucket": xb.size // 6}) as ctx:
    out["k_a"] = forward(ctx, xa)
    out["k_b"] = forward(ctx, xb)
w = np.random.default_rng(5).integers(2, 256, 100000).astype(np.uint8)
w[0] = 1
x = np.concatenate([w, w, w])
x[200000 + 70000] ^= 0x40
out["p_wide"] = case(x, bucket=x.size // 3)
out["p_narrow"] = case(x, wide=False)
print("FIGURES " + json.dumps(out, sort_keys=True))
print("stages ok")
""" % (ROOT, TESTS, KNOBS)


def run_child(timeout=600, lib=None):
    """CHILD in a process of its own; returns the figures of every case.  lib: another build of the library (the recording run)."""
    env = dict(os.environ, BWTS_TEST_CHILD="1", **ENV)
    for k in KNOBS:
        env.pop(k, None)
    if lib:
        env["BWTS_LIB_OVERRIDE"] = lib
    proc = subprocess.Popen([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT)
    try:
        out, _ = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        proc.kill()
        out, _ = proc.communicate()
        raise AssertionError("child timed out\n%s" % _child_report("wide stages", out))
    _wait_gpu_handle_released(proc.pid)
    text = out.decode(errors="replace")
    if proc.returncode != 0 or "stages ok" not in text:
        raise AssertionError("child: exit %d\n%s" % (proc.returncode, _child_report("wide stages", out)))
    return json.loads([ln for ln in text.splitlines() if ln.startswith("FIGURES ")][-1][8:]), text


@pytest.mark.gpu
def test_every_stage_does_what_the_parent_did_child():
    if os.environ.get("BWTS_TEST_CHILD"):
        pytest.skip("already inside a child run")
    got, _ = run_child()
    with open(FIXTURE) as f:
        want = json.load(f)["cases"]
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        for key in sorted(want[name]):
            assert got[name][key] == want[name][key], (name, key, got[name][key], want[name][key])
    # what the cases are there to reach, read off the parent's own record
    scatter = lambda c: want[c]["k"]["radix_scatter"][0]
    assert scatter("b") > scatter("b_ranks")                        # the direct run's sample sort came first, then the ranks run
    assert want["b"]["round_active"] == want["b_ranks"]["round_active"] and want["k_b"] == want["b"]
    assert scatter("c") > 5 * scatter("b_ranks")                    # dozens of parts a round
    assert want["f"]["rounds"] == 0 and want["f"]["active_after_round0"] > 0      # refused after the buckets
    assert want["g"]["lyndon_rounds"] > 0 and want["h"]["lyndon_rounds"] > 0 and want["a"]["lyndon_rounds"] == 0
    assert want["i"]["factors"] > 1000
    # a candidate scan, and the resolver launched again after every grid-wide comparison: 1 + (g + 1) + g launches for g >= 1 of them
    assert want["p_narrow"]["k"]["lyndon"][0] >= 4 and want["p_wide"]["factors"] == want["p_narrow"]["factors"]
