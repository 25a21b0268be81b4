"""bwts_forward_segments / bwts_inverse_segments: many independent inputs in one device pass.  Segment s of the output must be
exactly what the single-input transform gives for segment s alone (include/bwts.h)."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b


def _concat(segs):
    segs = [_u8(s) for s in segs]
    return np.concatenate(segs), np.array([s.size for s in segs], dtype=np.uint64)


def _per_segment(fn, data, lengths):
    out, off = [], 0
    for n in lengths:
        out.append(fn(data[off:off + int(n)]))
        off += int(n)
    return np.concatenate(out)


def _check_both(ctx, segs):
    data, lengths = _concat(segs)
    y = ctx.forward_segments(data, lengths)
    want = _per_segment(O.forward, data, lengths)
    assert np.array_equal(y, want)
    t = ctx.timings()
    assert t.n == data.size
    back = ctx.inverse_segments(y, lengths)
    assert np.array_equal(back, data)
    assert np.array_equal(back, _per_segment(O.inverse, y, lengths))
    return y


def _fib(n):
    a, b = "a", "ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n].encode()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_segment_symbols_exported(pkg):
    L = pkg.lib()
    for name in ("bwts_forward_segments", "bwts_inverse_segments", "bwts_forward_segments_device", "bwts_inverse_segments_device"):
        assert name in pkg.EXPORTS
        assert hasattr(L, name)


def test_segment_null_arguments_rejected(pkg):
    L = pkg.lib()
    one = (ctypes.c_uint64 * 1)(5)
    assert L.bwts_forward_segments(None, None, None, 0, None) == -1
    assert L.bwts_inverse_segments(None, None, one, 1, None) == -1
    assert L.bwts_forward_segments_device(None, None, one, 1, None) == -1
    assert L.bwts_inverse_segments_device(None, None, None, 0, None) == -1


# ---- GPU: hand cases -----------------------------------------------------------------------------------------------------------------

HAND = {
    "aba_c": [b"aba", b"c"],
    "tail_is_head_prefix": [b"abcab", b"z", b"abab", b"b"],
    "one_byte_each": [bytes([c]) for c in b"the quick brown fox jumps over the lazy dog"],
    "constant": [b"a" * 7, b"b" * 300, b"a" * 1, b"\x00" * 64],
    "identical": [b"banana"] * 9,
    "rotations": [b"abcde", b"cdeab", b"eabcd", b"bcdea"],
    "ba_k": [b"ba" * 50, b"ba" * 3, b"ab" * 17, b"bab"],
    "fibonacci": [_fib(233), _fib(1000), _fib(89)],
    "single_first": [b"q"] + [bytes(O.generate("text", 70000, 3))],
    "single_last": [bytes(O.generate("zipf", 90001, 4)), b"\x00"],
    "single_middle": [bytes(O.generate("dna", 65536, 5)), b"x", bytes(O.generate("uniform256", 40000, 6))],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_segments_hand_cases(ctx, name):
    _check_both(ctx, HAND[name])


@pytest.mark.gpu
def test_segments_aba_c_is_not_the_concatenation(ctx):
    """segment "aba" factors as ab|a on its own; read inside "abac" it would be one factor."""
    y = ctx.forward_segments(np.frombuffer(b"abac", dtype=np.uint8), [3, 1])
    assert bytes(y) == bytes(O.forward(b"aba")) + b"c"


# ---- GPU: random segmentations ----------------------------------------------------------------------------------------------------------

def _random_lengths(rng, total, lo, hi):
    out, left = [], total
    while left:
        n = int(min(left, rng.integers(lo, hi + 1)))
        out.append(n)
        left -= n
    return np.array(out, dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform256", "zipf", "dna", "text"])
@pytest.mark.parametrize("shape", ["tiny", "small", "mixed"])
def test_segments_random(ctx, kind, shape):
    rng = np.random.default_rng(["uniform256", "zipf", "dna", "text"].index(kind) * 3 + ["tiny", "small", "mixed"].index(shape))
    total = {"tiny": 20000, "small": 1 << 20, "mixed": 3 << 20}[shape]
    data = O.generate(kind, total, 11)
    if shape == "tiny":
        lengths = _random_lengths(rng, total, 1, 4)
    elif shape == "small":
        lengths = _random_lengths(rng, total, 1, 5000)
    else:
        lengths = _random_lengths(rng, total, 1, 400000)
    y = ctx.forward_segments(data, lengths)
    assert np.array_equal(y, _per_segment(O.forward, data, lengths))
    assert np.array_equal(ctx.inverse_segments(y, lengths), data)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("zipf", 1 << 20), ("dna", 300001), ("uniform256", 70000), ("text", 123457)])
def test_segments_count_one_equals_single(ctx, kind, n):
    x = O.generate(kind, n, 7)
    y = ctx.forward_segments(x, [n])
    assert np.array_equal(y, ctx.forward(x))
    assert np.array_equal(ctx.inverse_segments(y, [n]), ctx.inverse(y))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zipf", "text", "dna"])
def test_segments_skewed(ctx, kind):
    """Long segments beside one-byte ones: a segment of 2 MiB or more is transformed alone, the rest share one pass; the inverse picks
    single calls for the long ones."""
    x = O.generate(kind, (3 << 20) + (1 << 20) + 3, 23)
    lengths = np.array([3 << 20, 1, 1 << 20, 1, 1], dtype=np.uint64)
    y = ctx.forward_segments(x, lengths)
    assert np.array_equal(y, _per_segment(O.forward, x, lengths))
    assert np.array_equal(ctx.inverse_segments(y, lengths), x)
    c = np.full(2 << 20, ord("q"), dtype=np.uint8)          # a constant segment just below the line: the Duval wave's longest case
    c[-1] = ord("a")
    ls = np.array([(2 << 20) - 1, 1], dtype=np.uint64)
    assert np.array_equal(ctx.forward_segments(c, ls), _per_segment(O.forward, c, ls))


@pytest.mark.gpu
def test_segments_lengths_must_match_the_input(ctx):
    x = O.generate("zipf", 1000, 2)
    with pytest.raises(Exception):
        ctx.forward_segments(x, [600, 600])
    with pytest.raises(Exception):
        ctx.inverse_segments(x, [10])


# ---- GPU: host-buffer forms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_segments_in_place_unpinned_and_refused(ctx, pkg):
    data = O.generate("text", 3 << 20, 21)
    lengths = _random_lengths(np.random.default_rng(5), data.size, 1000, 200000)
    want = _per_segment(O.forward, data, lengths)
    buf = data.copy()                       # unpinned numpy memory, transformed in place
    ctx.forward_segments(buf, lengths, out=buf)
    assert np.array_equal(buf, want)
    ctx.inverse_segments(buf, lengths, out=buf)
    assert np.array_equal(buf, data)
    # refused calls leave out untouched
    L = pkg.lib()
    out = np.full(data.size, 0x77, dtype=np.uint8)
    bad = lengths.copy()
    bad[3] = 0
    assert L.bwts_forward_segments(ctx._h, data.ctypes.data, bad.ctypes.data, bad.size, out.ctypes.data) == -1
    over = np.array([1 << 63, 1 << 63], dtype=np.uint64)
    assert L.bwts_forward_segments(ctx._h, data.ctypes.data, over.ctypes.data, 2, out.ctypes.data) == -1
    big = np.array([1 << 32, 1], dtype=np.uint64)
    assert L.bwts_inverse_segments(ctx._h, data.ctypes.data, big.ctypes.data, 2, out.ctypes.data) == -5
    assert L.bwts_forward_segments(ctx._h, data.ctypes.data, lengths.ctypes.data, 0, out.ctypes.data) == -1
    assert np.all(out == 0x77)


@pytest.mark.gpu
def test_segments_device_alias_refused(ctx, pkg):
    n = 1 << 16
    d = ctx.alloc(2 * n)
    ctx.generate("zipf", 3, n, d)
    ls = np.array([n // 2, n // 2], dtype=np.uint64)
    L = pkg.lib()
    assert L.bwts_forward_segments_device(ctx._h, d.ptr, ls.ctypes.data, 2, d.ptr) == -1
    assert L.bwts_inverse_segments_device(ctx._h, d.ptr, ls.ctypes.data, 2, d.ptr + n // 2) == -1
    d.free()


# ---- GPU: at scale, on the device entry points ----------------------------------------------------------------------------------------

def _scale_case(ctx, kind, lengths, samples=6):
    n = int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    d_in, d_out, d_back, d_one = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(int(lengths.max()))
    try:
        ctx.generate(kind, 41, n, d_in)
        ctx.forward_segments_device(d_in, lengths, d_out)
        t = ctx.timings()
        assert t.n == n and t.factors >= lengths.size
        # every segment against a single-input call on that segment
        for s in range(lengths.size):
            a, ln = int(off[s]), int(lengths[s])
            ctx.forward_device(d_in.ptr + a, ln, d_one)
            assert ctx.device_equal(d_one, d_out.ptr + a, ln), "segment %d differs" % s
        # a sample against the CPU oracle, by sha-256
        x = d_in.download()
        y = d_out.download()
        rng = np.random.default_rng(lengths.size)
        for s in sorted(set([0, lengths.size - 1] + list(rng.integers(0, lengths.size, samples)))):
            a, b = int(off[s]), int(off[s + 1])
            assert hashlib.sha256(bytes(O.forward(x[a:b]))).digest() == hashlib.sha256(bytes(y[a:b])).digest()
        ctx.inverse_segments_device(d_out, lengths, d_back)
        assert ctx.device_equal(d_back, d_in, n)
    finally:
        for d in (d_in, d_out, d_back, d_one):
            d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zipf", "text"])
def test_segments_1gib_64k(ctx, kind):
    _scale_case(ctx, kind, np.full(16384, 1 << 16, dtype=np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zipf", "text"])
def test_segments_1gib_mixed(ctx, kind):
    rng = np.random.default_rng(9)
    ls = []
    left = 1 << 30
    while left:
        n = int(min(left, 1 << int(rng.integers(12, 21))))
        ls.append(n)
        left -= n
    _scale_case(ctx, kind, np.array(ls, dtype=np.uint64))


# ---- GPU: route switches, in a child process ------------------------------------------------------------------------------------------

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as ge, oracle_lib as O
pkg = ge.load_package()
with pkg.Context(0) as ctx:
    for kind in ("zipf", "text", "dna"):
        x = O.generate(kind, 1 << 20, 17)
        ls = np.array([1, 300000, 5, 4096, 2, (1 << 20) - 304104], dtype=np.uint64)
        y = ctx.forward_segments(x, ls)
        off = 0
        for n in ls:
            assert np.array_equal(y[off:off + int(n)], O.forward(x[off:off + int(n)])), kind
            off += int(n)
        assert np.array_equal(ctx.inverse_segments(y, ls), x), kind
print("ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("knob,big", [("BWTS_SEG_INV_BIG", "1"), ("BWTS_SEG_INV_BIG", "4097"), ("BWTS_SEG_FWD_BIG", "1"),
                                      ("BWTS_SEG_FWD_BIG", "4097")])
def test_segments_route_switch(knob, big):
    """BWTS_SEG_INV_BIG / BWTS_SEG_FWD_BIG move the length from which a segment takes the single-input inverse / forward on its own
    (1: every segment)."""
    env = dict(os.environ, BWTS_TEST_KNOBS="1")
    env[knob] = big
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode().strip().endswith("ok")
