"""GPU suite (-m gpu): the context's own account of its device memory (bwts_timings::device_bytes) against what the allocation
trace (BWTS_TRACE_ALLOC=1) shows live, after calls through the transforms' bracket and the entropy coder's, across a growth on a
live context and across bwts_ctx_release_memory.  Exact: byte counts and addresses, no tolerance.

The trace lines are those of csrc/ctx_memory.hip: `[bwts alloc] ctx P device + NAME [START, END) BYTES bytes` when the context takes
a block, `... device - [START, START) 0 bytes` when it gives one up.  The `small words` block is not part of device_bytes.  BWTS_GUARD
stays unset (a guarded block is not traced); the sizes reach neither the wide forward's tied-list blocks nor a one-call block, which
are not traced either."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_lib as O, mtf_model as M, ec_model as E, __graft_entry__ as ge
pkg = ge.load_package()

def mark(ctx, step):
    sys.stderr.write("[marker] %%s device_bytes=%%d\n" %% (step, ctx.timings().device_bytes))
    sys.stderr.flush()

x = O.generate("uniform256", 70001, 7)
want_x = O.forward(x)
lengths = np.array([1000, 1, 5000], dtype=np.uint64)
cuts = [0, 1000, 1001, 6001]
segs = x[:6001]
want_segs = np.concatenate([O.forward(segs[a:b]) for a, b in zip(cuts, cuts[1:])])
big = O.generate("zipf", 3 << 20, 7)
with pkg.Context(0) as ctx:
    assert np.array_equal(ctx.forward(x), want_x); mark(ctx, "1 forward")
    ys = ctx.forward_segments(segs, lengths)
    assert np.array_equal(ys, want_segs); mark(ctx, "2 forward_segments")
    assert np.array_equal(ctx.inverse_segments(ys, lengths), segs); mark(ctx, "2 inverse_segments")
    assert ctx.mtf_forward(x).tobytes() == M.forward_fast(x.tobytes()); mark(ctx, "3 mtf_forward")
    s = ctx.ec_encode(x)
    assert s.tobytes() == E.encode(x); mark(ctx, "4 ec_encode")
    assert np.array_equal(ctx.ec_decode(s), x); mark(ctx, "4 ec_decode")
    assert np.array_equal(ctx.forward(big), O.forward(big)); mark(ctx, "5 forward grown")
    ctx.release_memory()
    sys.stderr.write("[released]\n"); sys.stderr.flush()
    assert np.array_equal(ctx.forward(x), want_x); mark(ctx, "6 forward after release")
print("context memory ok")
"""

_ALLOC = re.compile(r"\[bwts alloc\] ctx \S+ device ([+-]) (.*?)\s*\[(0x[0-9a-f]+), (0x[0-9a-f]+)\) (\d+) bytes")
_MARK = re.compile(r"\[marker\] (.*) device_bytes=(\d+)")
_STEPS = ["1 forward", "2 forward_segments", "2 inverse_segments", "3 mtf_forward", "4 ec_encode", "4 ec_decode", "5 forward grown",
          "6 forward after release"]


def test_device_bytes_equals_the_live_blocks_of_the_trace():
    if os.environ.get("BWTS_TEST_CHILD"):
        pytest.skip("already inside a child run")
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, BWTS_TEST_CHILD="1", BWTS_TRACE_ALLOC="1")
    env.pop("BWTS_GUARD", None)
    from test_gpu_parity import _wait_gpu_handle_released
    proc = subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT)
    try:
        out, _ = proc.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        proc.kill()
        out, _ = proc.communicate()
    _wait_gpu_handle_released(proc.pid)
    text = out.decode(errors="replace")
    assert proc.returncode == 0 and "context memory ok" in text, text[-4000:]

    live = {}                   # start address -> (serial number of the trace line, name, bytes)
    seen, before_release, final, freed, freed_at = [], None, None, 0, {}
    for serial, line in enumerate(text.splitlines()):
        m = _ALLOC.search(line)
        if m:
            sign, name, start, end, size = m.group(1), m.group(2), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5))
            if sign == "+":
                assert end - start == size, line
                if name != "small words":
                    assert start not in live, (line, live[start])
                    live[start] = (serial, name, size)
            elif start in live:      # (the context's last free, at its end, is that of the small words)
                del live[start]
                freed += 1
            continue
        m = _MARK.search(line)
        if m:
            step, reported = m.group(1), int(m.group(2))
            print("%-26s device_bytes %12d, live in the trace %12d: %s" % (step, reported, sum(b[2] for b in live.values()),
                                                                         sorted((b[1], b[2]) for b in live.values())))
            assert reported == sum(b[2] for b in live.values()), (step, reported, sorted(live.values()))
            if step == "5 forward grown":
                before_release = {b[0] for b in live.values() if b[1].startswith(("side block", "device input", "device output"))}
            seen.append(step)
            freed_at[step], final = freed, dict(live)       # (behind the last marker the context is destroyed: everything goes)
        elif line.startswith("[released]"):
            # the segment table stays with the context; everything else device_bytes counts is gone
            assert [b[1] for b in live.values()] == ["segment table"], sorted(live.values())
    assert seen == _STEPS, seen
    # step 5 grew the arena and the input and output blocks on a live context: each gave its smaller block up first
    assert freed_at["5 forward grown"] - freed_at["4 ec_decode"] >= 3, freed_at
    assert before_release and not before_release & {b[0] for b in final.values()}, (before_release, sorted(final.values()))
    names = {b[1] for b in final.values()}
    assert {"arena", "device input 0", "device output 0", "segment table"} <= names, names
