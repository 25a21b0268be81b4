"""The compact form of the n > 2^32 inverse (wide_inverse.h): LF as packed 40-bit entries, segment records of one splitter spacing.
It is what inverts the wide forward's outputs beyond ~16 GiB, where the full form's ~13 n bytes do not fit the device.

A context reads its knobs when it is made, so every case that forces a form runs in a child process with the environment set: one at
a time, output kept, and nothing started after a child has died.  The last case (dna of 24 GiB, no knobs) runs in this process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import _child_report, _wait_gpu_handle_released

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
GIB = 1 << 30

HEAD = r"""
import os, sys, time, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_lib as O, __graft_entry__ as ge
pkg = ge.load_package()
""" % (ROOT, TESTS)

_child_failed = []


def _run_child(name, body, env_extra, timeout):
    if os.environ.get("BWTS_TEST_CHILD"):
        pytest.skip("already inside a child run")
    if _child_failed:
        pytest.fail("not started: child %s died before" % _child_failed[0])
    env = dict(os.environ, BWTS_TEST_CHILD="1", BWTS_TEST_KNOBS="1", BWTS_FORCE_WIDE="2", BWTS_WIDE_INV="compact", **env_extra)
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


@pytest.mark.gpu
def test_compact_small_vs_oracle_child():
    """Forced compact form on small inputs with small segments and slots (many overflow nodes): the inverse equals the oracle's on
    natural data (lengths not multiples of the splitter spacing), sorted runs (many tiny cycles), 1^b 0^c (one long cycle without a
    splitter: the unit-rank route), and once with the byte map instead of the moments."""
    body = r"""
def check(x, y, tag):
    with pkg.Context(0) as ctx:
        got = ctx.inverse(y)
        t = ctx.timings()
    assert np.array_equal(got, x), tag
    print(tag, "n", x.size, "factors", t.factors, "unvisited", t.unvisited)
    return t
for slot in ("64", "1024", "192"):
    os.environ["BWTS_WIDE_SLOT"] = slot
    for kind, n, seed in (("zipf", 300007, 1), ("dna", 200003, 2), ("uniform256", 100001, 3), ("text", 250013, 4), ("zipf", 1 << 20, 5)):
        x = O.generate(kind, n, seed)
        check(x, O.forward(x), "%s slot %s" % (kind, slot))
os.environ["BWTS_WIDE_SLOT"] = "64"
rng = np.random.default_rng(4242)
for rep in range(3):
    n = int(rng.integers(5000, 40000))
    x = np.sort(rng.integers(0, 100, size=n, dtype=np.uint8))[::-1].copy()
    c = int(rng.integers(0, n))
    x = (np.concatenate([x[c:], x[:c]]) + 48).astype(np.uint8)
    check(x, O.forward(x), "sorted run %d" % rep)
# B = 1^b 0^c sends i to i + c (mod n): with n = 2^k and c = 2 * odd, two cycles of n / 2 elements, the odd one free of
# multiples of 1024; at 2^20 that cycle is too long for one lane (the unit-rank route)
for n, c in ((1 << 17, 50002), (1 << 20, 2 * 177771)):
    B = np.concatenate([np.full(n - c, 1, np.uint8), np.zeros(c, np.uint8)])
    t = check(O.inverse(B), B, "long cycle without a splitter n %d" % n)
    assert t.unvisited >= n // 2
os.environ["BWTS_INV_MARK"] = "bytemap"
for kind, n, seed in (("zipf", 300007, 6), ("dna", 200003, 7)):
    x = O.generate(kind, n, seed)
    check(x, O.forward(x), "bytemap %s" % kind)
B = np.concatenate([np.full((1 << 20) - 2 * 177771, 1, np.uint8), np.zeros(2 * 177771, np.uint8)])
check(O.inverse(B), B, "bytemap long cycle")
# more unreached elements (2^21) than a fresh context's first collection holds (2^20): the marks are collected twice
for mark in ("bytemap", "moments"):
    os.environ["BWTS_INV_MARK"] = mark
    n, c = 1 << 22, 2 * 1234567
    B = np.concatenate([np.full(n - c, 1, np.uint8), np.zeros(c, np.uint8)])
    t = check(O.inverse(B), B, "%s long cycle, second collection" % mark)
    assert t.unvisited == n // 2
print("small ok")
"""
    _run_child("small", body, {"BWTS_WIDE_SEG_LOG2": "13"}, 900)


@pytest.mark.gpu
def test_compact_memory_bound_1gib_child():
    """Forced compact on zipf(2^30) after release_memory(): the inverse gives back the input and the context holds at most
    7.5 n + 1 GiB (the full form holds about 13 n)."""
    body = r"""
n = 1 << 30
os.environ.pop("BWTS_FORCE_WIDE"); os.environ.pop("BWTS_WIDE_INV")
a, b = None, None
with pkg.Context(0) as f:
    a, b = f.alloc(n), f.alloc(n)
    f.generate("zipf", 77, n, a)
    f.forward_device(a, n, b)
    os.environ["BWTS_FORCE_WIDE"] = "2"; os.environ["BWTS_WIDE_INV"] = "compact"
    with pkg.Context(0) as ctx:
        c = ctx.alloc(n)
        f.release_memory()
        ctx.release_memory()
        ctx.inverse_device(b, n, c)
        t = ctx.timings()
        assert ctx.device_equal(a, c, n)
        c.free()
    a.free(); b.free()
print("device_bytes %d = %.2f n, %.1f ms" % (t.device_bytes, t.device_bytes / n, t.total_ms))
assert t.device_bytes <= 7.5 * n + (1 << 30), t.device_bytes
print("bound ok")
"""
    _run_child("bound", body, {}, 600)


@pytest.mark.gpu
def test_compact_pinned_host_buffers_child():
    """Forced compact with input and output in pinned host blocks: equal to the main-path inverse."""
    body = r"""
n = 300 << 20
x = O.generate("dna", n, 31)
os.environ["BWTS_FORCE_WIDE"] = "0"
with pkg.Context(0) as f:
    y = f.forward(x)
os.environ["BWTS_FORCE_WIDE"] = "2"
with pkg.Context(0) as ctx:
    hin, pin = ctx.host_alloc(n)
    hout, pout = ctx.host_alloc(n)
    hin[:] = y
    ctx.inverse_device(pin, n, pout)
    assert np.array_equal(hout, x)
    ctx.host_free(pin); ctx.host_free(pout)
os.environ["BWTS_FORCE_WIDE"] = "0"
with pkg.Context(0) as m:
    assert np.array_equal(m.inverse(y), x)
print("pinned ok")
"""
    _run_child("pinned", body, {}, 900)


@pytest.mark.gpu
def test_compact_12gib_child(ctx):
    """Forced compact on dna(12 GiB) gives back the input (checked on the device against the generated input); prints both forms'
    times and device bytes."""
    ctx.release_memory()                  # what this process's context holds stays off the device while the child runs
    body = r"""
n = 12 << 30
os.environ.pop("BWTS_FORCE_WIDE"); os.environ.pop("BWTS_WIDE_INV")
f = pkg.Context(0)
x, y = f.alloc(n), f.alloc(n)
f.generate("dna", 5, n, x)
f.forward_device(x, n, y)
f.release_memory()
for form in ("compact", "full"):
    os.environ["BWTS_WIDE_INV"] = form
    ctx = pkg.Context(0)
    out = ctx.alloc(n)
    for call in ("first", "second"):                 # the second call finds its memory in place
        t0 = time.perf_counter()
        try:
            ctx.inverse_device(y, n, out)
        except pkg.BwtsError as e:
            # the full form (~14 n) is measured where it fits beside the buffers; not fitting is what the compact form is for
            if form == "full" and e.code == -3:
                print("full: does not fit (%s)" % e); break
            raise
        dt = time.perf_counter() - t0
        t = ctx.timings()
        assert ctx.device_equal(x, out, n), form
        print("%s, %s call: %.0f ms wall, %.0f ms device, device_bytes %.1f GiB = %.2f n, factors %d, unvisited %d" %
              (form, call, 1e3 * dt, t.total_ms, t.device_bytes / 2**30, t.device_bytes / n, t.factors, t.unvisited), flush=True)
    out.free(); ctx.close()
f.close()
print("12gib ok")
"""
    _run_child("12gib", body, {}, 1200)


@pytest.mark.gpu
def test_wide_round_trip_24gib(pkg, ctx):
    """dna(24 GiB) inverted with no knobs: the full form's ~13 n does not fit, the compact form takes over.  Nothing n-sized goes to
    the host: the result is compared on the device with the input regenerated from its seed."""
    n = 24 * GIB
    ctx.release_memory()
    c = pkg.Context(0)
    try:
        try:
            x, y = c.alloc(n), c.alloc(n)
        except pkg.BwtsError as e:
            pytest.skip("no room for the test's own buffers: %s" % e)
        c.generate("dna", 1, n, x)
        c.forward_device(x, n, y)
        fwd_factors = c.timings().factors
        x.free()
        c.release_memory()
        try:
            out = c.alloc(n)
        except pkg.BwtsError as e:
            pytest.skip("no room for the test's own buffers: %s" % e)
        c.inverse_device(y, n, out)
        t = c.timings()
        print("dna(24 GiB) inverse: %.0f ms device, device_bytes %.1f GiB = %.2f n" % (t.total_ms, t.device_bytes / GIB, t.device_bytes / n))
        assert t.factors == fwd_factors
        assert int(y.download(1)[0]) == int(O.generate("dna", 1, 1, off=n - 1)[0])
        y.free()
        x = c.alloc(n)
        c.generate("dna", 1, n, x)
        assert c.device_equal(x, out, n)
        x.free(); out.free()
    finally:
        c.close()
