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
import segment_cases as C

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

def _scale_case(ctx, kind, lengths, samples=6, data=None, factors=None):
    """kind: the device generator's input kind, or data: the input itself (host array).  factors: the expected factor count."""
    n = int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    d_in, d_out, d_back, d_one = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n), ctx.alloc(int(lengths.max()))
    try:
        if data is None:
            ctx.generate(kind, 41, n, d_in)
        else:
            d_in.upload(data)
        ctx.forward_segments_device(d_in, lengths, d_out)
        t = ctx.timings()
        assert t.n == n and t.factors >= lengths.size
        if factors is not None:
            assert t.factors == factors
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
        if factors is not None:
            assert ctx.timings().factors == factors
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


# ---- GPU: segments that share material (tests/segment_cases.py) ------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_segments_structured(ctx, name):
    """Copies, near copies, records, windows, powers: groups of equal infinite words across segments, whose members the shared pass must
    give exactly their own slots (a member twice and another missing moves a byte into the wrong segment)."""
    data, lengths = C.build(name)
    min_rounds = C.FAMILIES[name][1]
    factors = C.expected_factors(data, lengths)
    y = ctx.forward_segments(data, lengths)
    t = ctx.timings()
    print("[seg-stats] %s: segments %d bytes %d rounds %d active_after_round0 %d factors %d" % (
        name, lengths.size, data.size, t.rounds, t.active_after_round0, t.factors))
    assert np.array_equal(y, C.expected_forward(data, lengths))
    assert t.n == data.size
    assert t.factors == factors
    if min_rounds is None:
        # one byte value overall: the constant-input shortcut, the identity with every position a factor
        assert np.array_equal(y, data) and t.factors == data.size and t.active_after_round0 == 0
    else:
        # (the case reaches the rounds: a change that stops it from doing so fails here rather than testing less)
        assert t.active_after_round0 > 0
        assert t.rounds >= min_rounds
    back = ctx.inverse_segments(y, lengths)
    assert np.array_equal(back, data)
    assert ctx.timings().factors == factors         # one cycle of the inverse per Lyndon factor of its output


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_segments_structured_inverse(ctx, name):
    """The same sets fed straight to the inverse (they are not forward outputs): long LF cycles and many tiny ones."""
    data, lengths = C.build(name)
    want = C.expected_inverse(data, lengths)
    x = ctx.inverse_segments(data, lengths)
    assert np.array_equal(x, want)
    assert ctx.timings().factors == C.expected_factors(want, lengths)


@pytest.mark.gpu
def test_segments_256mib_copies(ctx):
    """3 documents of 16 KiB, 5461 copies each (groups of 5461 in the big list), through the device entry points."""
    data, lengths = C.copies(201, 16 << 10, 5461)
    _scale_case(ctx, None, lengths, data=data, factors=C.expected_factors(data, lengths))


@pytest.mark.gpu
def test_segments_256mib_windows(ctx):
    """16 384 windows of 16 KiB at a step of 4 KiB, through the device entry points."""
    data, lengths = C.windows(202, 16 << 10, 4 << 10, 16384)
    _scale_case(ctx, None, lengths, data=data, factors=C.expected_factors(data, lengths))


# ---- GPU: the tie classes the shared pass reaches, shown by the round trace ---------------------------------------------------------------

TRACE_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as ge, segment_cases as C
pkg = ge.load_package()
with pkg.Context(0) as ctx:
    for name in %(names)r:
        data, lengths = C.build(name)
        sys.stderr.write("[case] %%s\n" %% name)
        sys.stderr.flush()
        y = ctx.forward_segments(data, lengths)
        assert np.array_equal(y, C.expected_forward(data, lengths)), name
        sys.stderr.flush()
print("ok")
"""


def _trace_classes(text):
    import re
    seen = {"big list": 0, "leave the big list": 0, "chunk rounds": 0, "groups <= 256": 0, "groups 257-2048": 0, "no split": 0}
    for line in text.splitlines():
        m = re.match(r"\[chunks\] list \d+: in chunks \d+ .*, big list (\d+)$", line)
        if m:
            seen["big list"] += int(m.group(1)) > 0
        m = re.match(r"\[chunks\] groups of up to \d+ members leave the big list at once: (\d+) elements", line)
        if m:
            seen["leave the big list"] += int(m.group(1)) > 0
        m = re.match(r"\[chunks\] round \d+ h \d+: .*leaves (\d+)$", line)
        if m:
            seen["chunk rounds"] += 1
            seen["leave the big list"] += int(m.group(1)) > 0
        m = re.match(r"\[chunks\] before round \d+, chunk elements by group size: .* 65-256: (\d+)  257-2048: (\d+)$", line)
        if m:
            seen["groups <= 256"] += int(m.group(1)) > 0
            seen["groups 257-2048"] += int(m.group(2)) > 0
        m = re.match(r"\[(chunks|rounds)\] round \d+: no group split, (\d+) elements left", line)
        if m:
            seen["no split"] += int(m.group(2)) > 0
    return seen


@pytest.mark.gpu
def test_segments_tie_classes_reached():
    """BWTS_ROUND_TRACE=1 on the copies and periodic sets: between them they reach a non-empty big list (groups of more than 2048
    equal infinite words), groups leaving it, the chunk rounds with groups of up to 256 (LDS counting) and of 257 .. 2048 (WIDE chunks),
    and a last round that splits no group -- the run ends with groups of equal infinite words left, whose members take their slots."""
    names = ["copies_16k_x200", "copies_4k_x1000", "copies_1k_x3000", "periodic"]
    env = dict(os.environ, BWTS_TEST_KNOBS="1", BWTS_ROUND_TRACE="1")
    code = TRACE_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "names": names}
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-3000:]
    assert r.stdout.decode().strip().endswith("ok")
    seen = _trace_classes(err)
    print("[seg-trace] %s" % seen)
    assert all(seen.values()), (seen, err[-3000:])


# ---- GPU: the partition's pass count (8 bits of segment id per pass) ------------------------------------------------------------------------

_TABLES = {}


def _tiny_table(which):
    if which not in _TABLES:
        _TABLES[which] = C.TinyTable(O.forward if which == "forward" else O.inverse)
    return _TABLES[which]


PASS_COUNTS = [2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("count", PASS_COUNTS, ids=lambda c: "count%d-passes%d" % (c, C.partition_passes(c)))
def test_segments_partition_passes(ctx, count):
    """count segments of 1 .. 3 bytes: the stable partition by segment id runs 1, 1, 2, 2, 3, 3 and 4 passes.  The two largest go through
    the device entry points, the others through the host forms."""
    data, lengths = C.tiny_segments(count, count)
    fwd, inv = _tiny_table("forward"), _tiny_table("inverse")
    want = fwd.apply(data, lengths)
    factors = fwd.count_factors(data, lengths)
    want_inv = inv.apply(data, lengths)
    inv_factors = fwd.count_factors(want_inv, lengths)
    if count < (1 << 24):
        y = ctx.forward_segments(data, lengths)
        assert ctx.timings().factors == factors
        assert np.array_equal(y, want)
        assert np.array_equal(ctx.inverse_segments(y, lengths), data)
        assert ctx.timings().factors == factors
        assert np.array_equal(ctx.inverse_segments(data, lengths), want_inv)
        assert ctx.timings().factors == inv_factors
        return
    n = data.size
    d_in, d_out, d_back = ctx.alloc(n), ctx.alloc(n), ctx.alloc(n)
    try:
        d_in.upload(data)
        ctx.forward_segments_device(d_in, lengths, d_out)
        assert ctx.timings().factors == factors
        assert np.array_equal(d_out.download(), want)
        ctx.inverse_segments_device(d_out, lengths, d_back)
        assert ctx.timings().factors == factors
        assert ctx.device_equal(d_back, d_in, n)
        ctx.inverse_segments_device(d_in, lengths, d_back)
        assert ctx.timings().factors == inv_factors
        assert np.array_equal(d_back.download(), want_inv)
    finally:
        for d in (d_in, d_out, d_back):
            d.free()


# ---- CPU: the helpers of tests/segment_cases.py ----------------------------------------------------------------------------------------------

SMALL_FAMILIES = {
    "copies": lambda s: C.copies(s, 300, 7),
    "near_copies": lambda s: C.near_copies(s, 300, 7),
    "records": lambda s: C.records(s, 20, 500),
    "windows": lambda s: C.windows(s, 400, 37, 20),
    "periodic": lambda s: C.periodic(s, per_word=5, kmax=40),
    "periodic_one": lambda s: C.periodic_one(s, b"abb", 5000, kmax=300),
    "powers": lambda s: C.powers(s, wlen=30, kmax=12),
    "constant": lambda s: C.constant(s, total=5000, hi=300),
    "mixed_route": lambda s: C.mixed_route(s, doc_len=256, r=5, long_len=3000),
    "tiny": lambda s: C.tiny_segments(s, 3000),
}


@pytest.mark.parametrize("family", sorted(SMALL_FAMILIES))
def test_segment_cases_deterministic(family):
    a, la = SMALL_FAMILIES[family](7)
    b, lb = SMALL_FAMILIES[family](7)
    assert a.dtype == np.uint8 and la.dtype == np.uint64 and int(la.sum()) == a.size and (la > 0).all()
    assert np.array_equal(a, b) and np.array_equal(la, lb)
    c, lc = SMALL_FAMILIES[family](8)
    assert not (np.array_equal(a, c) and np.array_equal(la, lc))


@pytest.mark.parametrize("family", sorted(SMALL_FAMILIES))
def test_segment_cases_expected_equals_direct_oracle(family):
    data, lengths = SMALL_FAMILIES[family](3)
    segs = C.split(data, lengths)
    assert np.array_equal(C.expected_forward(data, lengths), np.concatenate([O.forward(s) for s in segs]))
    assert np.array_equal(C.expected_inverse(data, lengths), np.concatenate([O.inverse(s) for s in segs]))
    assert C.expected_factors(data, lengths) == sum(len(O.lyndon_starts(s)) for s in segs)


def test_segment_cases_tiny_table_equals_direct_oracle():
    fwd, inv = _tiny_table("forward"), _tiny_table("inverse")
    for seed in range(3):
        data, lengths = C.tiny_segments(seed, 2000)
        segs = C.split(data, lengths)
        assert np.array_equal(fwd.apply(data, lengths), np.concatenate([O.forward(s) for s in segs]))
        assert np.array_equal(inv.apply(data, lengths), np.concatenate([O.inverse(s) for s in segs]))
        assert fwd.count_factors(data, lengths) == sum(len(O.lyndon_starts(s)) for s in segs)
        assert set(np.unique(data)) <= set(C.TINY_ALPHABET) and {0x00, 0xFF} <= set(np.unique(data))
        assert set(np.unique(lengths)) == {1, 2, 3}


def test_segment_cases_partition_passes():
    assert [C.partition_passes(c) for c in PASS_COUNTS] == [1, 1, 2, 2, 3, 3, 4]


def _is_lyndon(w):
    return all(w < w[i:] + w[:i] for i in range(1, len(w)))


def test_segment_cases_families_have_their_property():
    # copies: r copies of each of ndocs documents
    data, lengths = C.copies(1, 300, 7, ndocs=3)
    _, counts = np.unique([s.tobytes() for s in C.split(data, lengths)], return_counts=True)
    assert sorted(counts) == [7, 7, 7]
    # near copies: every copy distinct from its document in one or two bytes, all of one length
    data, lengths = C.near_copies(1, 300, 7, ndocs=2)
    segs = C.split(data, lengths)
    assert len({s.tobytes() for s in segs}) > 7 and set(lengths) == {300}
    dist = [min(int((s != t).sum()) for t in segs if t is not s) for s in segs]
    assert max(dist) <= 4
    # records: one shared header, tails of 16 .. 256 bytes
    data, lengths = C.records(1, 20, 500)
    segs = C.split(data, lengths)
    assert all(np.array_equal(s[:500], segs[0][:500]) for s in segs)
    assert all(16 <= len(s) - 500 <= 256 for s in segs)
    # windows: neighbours overlap by L - step bytes
    data, lengths = C.windows(1, 400, 37, 20)
    segs = C.split(data, lengths)
    assert all(np.array_equal(segs[i][37:], segs[i + 1][:400 - 37]) for i in range(19))
    # periodic: every segment is u^k or u^k.v, v a proper prefix of a Lyndon word u
    assert all(_is_lyndon(u) for u in C.LYNDON_WORDS)
    data, lengths = C.periodic(1, per_word=5, kmax=40)
    for s in C.split(data, lengths):
        b = s.tobytes()
        assert any(b[:len(u) * (len(b) // len(u))] == u * (len(b) // len(u)) and u.startswith(b[len(u) * (len(b) // len(u)):])
                   for u in C.LYNDON_WORDS)
    data, lengths = C.periodic_one(1, b"ab", 5000, kmax=300)
    assert all(s.tobytes() == b"ab" * (len(s) // 2) for s in C.split(data, lengths)) and data.size == 5000
    # powers: w^k and rotations of w
    data, lengths = C.powers(1, wlen=30, kmax=12)
    segs = sorted((s.tobytes() for s in C.split(data, lengths)), key=len)
    w = segs[-1][:30]
    assert segs[31:] == [w * k for k in range(2, 13)] and set(segs[:31]) == {w[i:] + w[:i] for i in range(30)}
    # constant: one byte value
    data, lengths = C.constant(1, total=5000, hi=300)
    assert np.unique(data).size == 1 and lengths.size > 1
    # mixed route: one segment of at least 2 MiB at the default size, made of the short segments' documents
    data, lengths = C.mixed_route(1, doc_len=256, r=5, long_len=3000)
    segs = C.split(data, lengths)
    long_seg = max(segs, key=len).tobytes()
    docs = {s.tobytes() for s in segs if len(s) == 256}
    assert len(docs) == 2 and all(long_seg[i:i + 256] in docs for i in range(0, 3000 - 256, 256))
    data, lengths = C.build("mixed_route")
    assert (lengths >= C.SEG_FWD_BIG).sum() == 1 and (lengths < C.SEG_FWD_BIG).sum() > 1


# ---- GPU: segments under the alternate sort modes, one child process per mode (kept last: a child that dies stops the rest) -----------------

ALT_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as ge, segment_cases as C
pkg = ge.load_package()
cases = {
    "copies": lambda: C.copies(301, 4 << 10, 300),
    "copies_big_groups": lambda: C.copies(302, 256, 3000, ndocs=2),
    "near_copies": lambda: C.near_copies(303, 1 << 10, 1000),
    "windows": lambda: C.windows(304, 2048, 7, 1500),
    "periodic": lambda: C.periodic(305, per_word=60, kmax=1500),
    "periodic_ab": lambda: C.periodic_one(306, b"ab", 4 << 20),
    "tiny": lambda: C.tiny_segments(307, 70000),
}
with pkg.Context(0) as ctx:
    for name, build in cases.items():
        data, lengths = build()
        y = ctx.forward_segments(data, lengths)
        assert np.array_equal(y, C.expected_forward(data, lengths)), name
        assert ctx.timings().factors == C.expected_factors(data, lengths), name
        assert np.array_equal(ctx.inverse_segments(y, lengths), data), name
print("ok")
"""

SEG_ALT_ENVS = [
    {"BWTS_DENSE": "tiles"},
    {"BWTS_VARLEN": "1", "BWTS_KEY_BITS": "24"},
    {"BWTS_VARLEN": "0", "BWTS_KEY_SYMBOLS": "2"},
    {"BWTS_RX_SMALL": "0"},
    {"BWTS_RX_PACK": "0"},
    {"BWTS_POISON": "1"},
]
_seg_alt_died = []


@pytest.mark.gpu
@pytest.mark.parametrize("env", SEG_ALT_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_segments_alternate_modes(env):
    """The structured sets (a few MiB each) under every sort mode that touches the shared pass, one child at a time (a context reads
    its knobs once).  After a child that ended by a signal or ran out of time, the later ones are not started."""
    if _seg_alt_died:
        pytest.fail("not started: an earlier child died (%s)" % _seg_alt_died[0])
    code = ALT_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BWTS_TEST_KNOBS="1", **env), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
    except subprocess.TimeoutExpired:
        _seg_alt_died.append("%s: time limit" % env)
        raise
    if r.returncode < 0:
        _seg_alt_died.append("%s: signal %d" % (env, -r.returncode))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    assert r.stdout.decode().strip().endswith("ok")
