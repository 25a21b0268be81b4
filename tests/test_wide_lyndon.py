"""The suffix route to the Lyndon factors of the n > 2^32 forward (wide_path.h): the blocked 64-bit sort run on suffixes, whose ISA's
strict prefix minima are the factor starts.  It takes the inputs whose factors the candidate search cannot settle -- runs of the smallest
byte make every later position followed by as many of it a candidate -- which the wide forward refused with BWTS_E_RANGE before.

A context reads its knobs when it is made, so every case that forces a route runs in a child process with the environment set: one at
a time, output kept, and nothing started after a child has died.  The last case (n = 2^32 + 2^28, no knobs) runs in this process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lyndon_blocks as LB
import oracle_lib as O
from test_gpu_parity import WIDE_CASES, _child_report, _wait_gpu_handle_released
from test_oracle import KAT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

HEAD = r"""
import os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_lib as O, lyndon_blocks as LB, __graft_entry__ as ge
pkg = ge.load_package()

def wide_forward(x, **knobs):
    # forced wide (BWTS_FORCE_WIDE=2 in the environment) with these knobs; the main path's inverse must give x back
    saved = {k: os.environ.get(k) for k in knobs}
    os.environ.update({k: str(v) for k, v in knobs.items()})
    try:
        with pkg.Context(0) as ctx:
            y = ctx.forward(x)
            t = ctx.timings()
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    forced = os.environ.pop("BWTS_FORCE_WIDE")
    try:
        with pkg.Context(0) as ctx:
            back = ctx.inverse(y)
    finally:
        os.environ["BWTS_FORCE_WIDE"] = forced
    return y, t, back

def check(tag, x, **knobs):
    y, t, back = wide_forward(x, **knobs)
    assert np.array_equal(y, O.forward(x)), tag
    k = len(O.lyndon_starts(x))
    assert t.factors == k, (tag, t.factors, k)
    assert t.lyndon_rounds > 0, tag
    assert np.array_equal(back, x), tag
    print(tag, "n", x.size, "factors", t.factors, "suffix rounds", t.lyndon_rounds, "rounds", t.rounds, "tied", t.active_after_round0)
""" % (ROOT, TESTS)

_child_failed = []


def _run_child(name, body, env_extra, timeout):
    if os.environ.get("BWTS_TEST_CHILD"):
        pytest.skip("already inside a child run")
    if _child_failed:
        pytest.fail("not started: child %s died before" % _child_failed[0])
    env = dict(os.environ, BWTS_TEST_CHILD="1", BWTS_TEST_KNOBS="1", BWTS_FORCE_WIDE="2", **env_extra)
    for k in ("BWTS_WIDE_LYNDON", "BWTS_WIDE_BUCKET", "BWTS_WIDE_PART", "BWTS_WIDE_DIRECT"):
        env.pop(k, None)
    proc = subprocess.Popen([sys.executable, "-c", HEAD + body], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT)
    try:
        out, _ = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        proc.kill()
        out, _ = proc.communicate()
        _child_failed.append(name)
        raise AssertionError("child %s timed out\n%s" % (name, _child_report(name, out)))
    _wait_gpu_handle_released(proc.pid)
    text = out.decode(errors="replace")
    print(text)
    if proc.returncode != 0 or (name + " ok") not in text:
        if proc.returncode < 0 or proc.returncode in (134, 139):
            _child_failed.append(name)
        raise AssertionError("child %s: exit %d\n%s" % (name, proc.returncode, _child_report(name, out)))
    return text


def test_inputs_have_the_shape_they_claim():
    """(CPU) The Lyndon-block input factors into exactly its blocks, and both zero-run inputs hold far more positions tied with the
    running key minimum than the candidate search takes (65 536)."""
    x, starts = LB.small_lyndon_blocks()
    assert np.array_equal(O.lyndon_starts(x), starts) and starts.size == 3000
    assert LB.positions_before_zero_runs(x, 17) > 100000
    t = LB.tar_like(1500, 5)
    assert LB.positions_before_zero_runs(t, 64) >= 100000
    y, s2 = LB.lyndon_blocks(500, 65 + np.arange(500) // 7, 200, 2000, 3)
    assert np.array_equal(O.lyndon_starts(y), s2)


@pytest.mark.gpu
def test_zero_runs_forced_wide_vs_oracle_child():
    """Forced wide (no fallback) with small segments, buckets and parts: the suffix route gives the oracle's factors and bytes on
    Lyndon blocks, tar-like data, a descending sort (one-symbol factors), a^n (the identity) and (ab)^m (b^m a^m); the candidate search
    alone -- the default below 2^32 -- still refuses the Lyndon blocks with BWTS_E_RANGE."""
    body = r"""
x, starts = LB.small_lyndon_blocks()
n = x.size
check("lyndon blocks", x, BWTS_WIDE_LYNDON="auto", BWTS_WIDE_BUCKET=n // 2, BWTS_WIDE_PART=n // 2)
check("lyndon blocks, tblocks of 2^12", x, BWTS_WIDE_LYNDON="auto", BWTS_WIDE_BUCKET=n // 2, BWTS_WIDE_PART=n // 2, BWTS_WIDE_TBLOCK_LOG2=12,
      BWTS_WIDE_DIRECT=0)
for lyn in (None, "candidates"):
    try:
        wide_forward(x, **({"BWTS_WIDE_LYNDON": lyn} if lyn else {}))
        raise AssertionError("the candidate search alone took the Lyndon blocks (%s)" % lyn)
    except pkg.BwtsError as e:
        assert e.code == -5, e
t = LB.tar_like(1500, 5)
check("tar-like", t, BWTS_WIDE_LYNDON="auto", BWTS_WIDE_BUCKET=t.size // 2, BWTS_WIDE_PART=t.size // 2)
rng = np.random.default_rng(3)
d = np.sort(rng.integers(0, 256, 200000).astype(np.uint8))[::-1].copy()
check("descending sort", d, BWTS_WIDE_LYNDON="auto", BWTS_WIDE_BUCKET=20000, BWTS_WIDE_PART=5000)
a = np.full(100000, ord("a"), np.uint8)
y, tm, back = wide_forward(a, BWTS_WIDE_LYNDON="suffix", BWTS_WIDE_BUCKET=a.size)
assert np.array_equal(y, a) and tm.factors == a.size and tm.lyndon_rounds > 0 and np.array_equal(back, a)
m = 100000
ab = np.tile(np.frombuffer(b"ab", np.uint8), m)
want = np.concatenate([np.full(m, ord("b"), np.uint8), np.full(m, ord("a"), np.uint8)])
y, tm, back = wide_forward(ab, BWTS_WIDE_LYNDON="auto", BWTS_WIDE_BUCKET=ab.size)
assert np.array_equal(y, want) and tm.factors == m and tm.lyndon_rounds > 0 and np.array_equal(back, ab)
assert np.array_equal(want, O.forward(ab))
print("zero runs ok")
"""
    _run_child("zero runs", body, {"BWTS_WIDE_SEG_LOG2": "13"}, 1200)


def _kats():
    out = [t.encode() for t, _ in KAT["text_to_bwts"]] + [bytes.fromhex(h) for h, _ in KAT["hex_to_bwts"]]
    return [k for k in out if len(k) >= 2] + [bytes(range(256)), bytes(range(255, -1, -1))]


@pytest.mark.gpu
def test_suffix_route_on_ordinary_data_child():
    """BWTS_WIDE_LYNDON=suffix on the wide path's ordinary cases and the known answers: same bytes and factor count as the oracle,
    so the two routes to the factors agree where both apply."""
    body = r"""
for kind, n, seed in %r:
    x = O.generate(kind, n, seed)
    check("suffix %%s" %% kind, x, BWTS_WIDE_LYNDON="suffix", BWTS_WIDE_BUCKET=max(256, n // 6))
for kat in %r:
    x = np.frombuffer(kat, np.uint8).copy()
    check("suffix kat %%r" %% kat[:16], x, BWTS_WIDE_LYNDON="suffix", BWTS_WIDE_BUCKET=256)
print("ordinary ok")
""" % (WIDE_CASES, _kats())
    _run_child("ordinary", body, {"BWTS_WIDE_SEG_LOG2": "13"}, 1200)


@pytest.mark.gpu
def test_lyndon_blocks_beyond_2p32(ctx, pkg):
    """n = 2^32 + 2^28 of Lyndon blocks (L = 65 + i / 2^16 zeros, bodies of 200..2000 bytes: millions of candidates), no knobs: the
    forward succeeds (it returned BWTS_E_RANGE before), finds exactly the blocks as factors, permutes the bytes with bwts[0] = T[n-1],
    and the wide inverse gives the input back."""
    x, starts = LB.big_lyndon_blocks((1 << 32) + (1 << 28))
    n, k = x.size, starts.size
    assert n > (1 << 32)
    del starts
    ctx.release_memory()            # (the shared context may still hold the arenas of earlier large cases)
    bufs = []
    try:
        try:
            bufs = [ctx.alloc(n), ctx.alloc(n)]
        except pkg.BwtsError:
            pytest.skip("not enough device memory")
        d_in, d_out = bufs
        d_in.upload(x)
        try:
            ctx.forward_device(d_in, n, d_out)
        except pkg.BwtsError as e:
            if e.code == -3:
                pytest.skip("not enough free device memory for the 4.25 GiB case")
            raise
        t = ctx.timings()
        print("forward %.0f ms, factors %d, suffix rounds %d, rounds %d, device GiB %.1f" % (t.total_ms, t.factors, t.lyndon_rounds, t.rounds,
                                                                                            t.device_bytes / 2**30))
        assert t.factors == k and t.lyndon_rounds > 0
        y = d_out.download()
        assert y[0] == x[-1]
        B = 1 << 28
        hx, hy = np.zeros(256, np.int64), np.zeros(256, np.int64)
        for o in range(0, n, B):
            hx += np.bincount(x[o:o + B], minlength=256)
            hy += np.bincount(y[o:o + B], minlength=256)
        assert np.array_equal(hx, hy)
        del y
        bufs.append(ctx.alloc(n))
        ctx.inverse_device(d_out, n, bufs[2])
        assert ctx.device_equal(d_in, bufs[2], n)
    finally:
        for b in bufs:
            b.free()
