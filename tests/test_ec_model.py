"""CPU suite of the entropy coder (include/bwts_ec.h): the model (tests/ec_model.py) against answers written out by hand, its round
trip, bound and cross-entropy inequality on every boundary size and content; the library's host arithmetic against the model; and
the stand-alone host program over the shared plan and validation header, built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ec_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, K = E.T, E.K
SIZES = [1, 2, 15, 16, 17, 1023, 1024, 1025, T - 1, T, T + 1, K * T - 1, K * T, K * T + 1, 2 * K * T + T + 7]


def contents(n, seed=0):
    """The inputs of the issue, by name: one repeated byte (f = 4096, nothing emitted), uniform bytes (expansion, near the bound),
    geometric ranks, 98 % zeros, zeros with about 180 rare symbols (the d < 0 loop), and two symbols at 1 : 10^5 (the f = 1 bump)."""
    rng = np.random.default_rng(1000 + seed)
    rare = np.zeros(n, dtype=np.uint8)
    for at in range(0, n, K * T):              # per block: 180 symbols, three times each where the block is long enough
        m = min(K * T, n - at)
        k = min(540, m // 4)
        rare[at + rng.choice(m, k, replace=False)] = 1 + (np.arange(k) % 180)
    two = np.zeros(n, dtype=np.uint8)
    two[99999::100000] = 200
    if n < 100000:
        two[n // 2] = 200
    sparse = np.where(rng.random(n) < 0.98, 0, rng.integers(0, 256, n)).astype(np.uint8)
    return {
        "repeat": np.full(n, 0x5A, dtype=np.uint8),
        "uniform": rng.integers(0, 256, n, dtype=np.uint8),
        "geometric": np.minimum(rng.geometric(0.3, n) - 1, 255).astype(np.uint8),
        "zeros98": sparse,
        "rare180": rare,
        "two_1e5": two,
    }


def _words(*vals):
    return b"".join(struct.pack("<I", v) for v in vals)


def test_known_answer_one_byte():
    """n = 1: one block, one tile, the byte's frequency 4096; f = 4096 never emits and leaves the state where it was."""
    table = bytearray(512)
    table[2 * 0x41:2 * 0x41 + 2] = struct.pack("<H", 4096)
    want = _words(0x43455742, 14 | 4 << 8 | 12 << 16, 1, 0) + bytes(table) + _words(256, 0, 0, 0) + _words(*([65536] * 64))
    assert E.encode(b"A") == want and len(want) == 800
    assert E.decode(want) == b"A"


def test_known_answer_four_bytes():
    """bytes([0, 0, 1, 0]): f[0] = 3072, f[1] = 1024, c = 0, 3072.  All four positions are lane 0, steps 0 .. 3; the encoder runs them
    backwards from 65536: step 3 (s = 0) 21 * 4096 + 1024 = 87040; step 2 (s = 1) 85 * 4096 + 0 + 3072 = 351232; step 1 (s = 0)
    114 * 4096 + 1024 = 467968; step 0 (s = 0) 152 * 4096 + 1024 = 623616.  No state reaches f * 2^20: no words."""
    table = struct.pack("<HH", 3072, 1024) + bytes(508)
    want = _words(0x43455742, 14 | 4 << 8 | 12 << 16, 4, 0) + table + _words(256, 0, 0, 0) + _words(623616, *([65536] * 63))
    assert E.encode(bytes([0, 0, 1, 0])) == want
    assert E.decode(want) == bytes([0, 0, 1, 0])


def test_normalise_rules():
    h = np.zeros(256, dtype=np.int64)
    h[[0, 1, 2]] = 1
    assert E.normalise(h)[:3].tolist() == [1366, 1365, 1365]                  # d > 0: once, to the lowest of the largest
    h[:] = 0
    h[0], h[200] = 100000, 1
    f = E.normalise(h)
    assert f[0] == 4095 and f[200] == 1                                         # the f = 1 bump
    h[:] = 0
    h[:180] = 3
    h[255] = K * T - 540
    f = E.normalise(h)
    assert f[:180].tolist() == [1] * 180 and f[255] == 4096 - 180 and f.sum() == 4096      # d = -171, all from the largest


@pytest.mark.parametrize("n", SIZES)
def test_round_trip_bound_and_cross_entropy(n):
    for name, x in contents(n, n % 97).items():
        s = E.encode(x)
        nt = E.tiles(n)
        nb = E.blocks(nt)
        assert len(s) % 16 == 0 and len(s) <= E.bound(n), name
        fixed = 16 + 512 * nb + E.pad16(4 * nt)
        bits = E.cross_entropy_bits(x)
        assert len(s) <= fixed + 272 * nt + int(np.ceil(bits / 8)), (name, len(s), bits)
        assert E.decode(s) == x.tobytes(), name
        if name == "repeat":
            assert len(s) == fixed + 256 * nt               # nothing emitted
        if name == "uniform" and n >= T:
            assert len(s) > n                               # the expansion path


def test_rare_symbols_take_the_minus_loop_often():
    """The rare180 content makes d < 0 by more than the largest frequency among the non-zero symbols."""
    x = contents(K * T, 0)["rare180"]
    h = np.bincount(x, minlength=256)
    first = np.where(h > 0, np.maximum(1, h * 4096 // h.sum()), 0)
    assert 4096 - int(first.sum()) < -int(first[1:].max())
    assert np.count_nonzero(h) == 181


def test_segments_are_single_streams():
    rng = np.random.default_rng(5)
    lengths = [T - 1, 1, T + 1, 3 * T + 5, 2]
    x = np.minimum(rng.geometric(0.4, sum(lengths)) - 1, 255).astype(np.uint8)
    streams = E.encode_segments(x, lengths)
    at = 0
    for ln, s in zip(lengths, streams):
        assert s == E.encode(x[at:at + ln]) and len(s) % 16 == 0
        at += ln
    sb = [len(s) for s in streams]
    assert E.decode_segments(b"".join(streams), sb, lengths) == x.tobytes()
    assert sum(sb) <= E.bound_segments(lengths)
    wrong = list(lengths)
    wrong[2] -= 1
    wrong[3] += 1
    assert E.decode_segments(b"".join(streams), sb, wrong) is None


def _put32(s, at, v):
    return s[:at] + struct.pack("<I", v) + s[at + 4:]


def malformed_cases(x):
    """(name, stream) for every malformed stream of the issue, made from the valid stream of x (at least two blocks, and a last tile
    that emits words); shared with the GPU suite, which must see each refused by the model first."""
    s = E.encode(x)
    n = len(x)
    nt, nb = E.tiles(n), E.blocks(E.tiles(n))
    dir_at = 16 + 512 * nb
    fixed = dir_at + E.pad16(4 * nt)
    sizes = np.frombuffer(s[dir_at:dir_at + 4 * nt], dtype="<u4").astype(np.int64)
    offs = fixed + np.concatenate(([0], np.cumsum(sizes)))
    cases = [
        ("wrong magic", _put32(s, 0, 0x43455743)),
        ("wrong params", _put32(s, 4, 14 | 4 << 8 | 11 << 16)),
        ("cut by 16", s[:-16]),
        ("cut to 15", s[:15]),
        ("cut inside the directory", s[:dir_at + 16]),
        ("table summing to 4095", s[:16 + 512] + _table_minus_one(s[16 + 512:16 + 1024]) + s[16 + 1024:]),
        ("tile size 240", _put32(s, dir_at + 4, 240)),
        ("tile size 264", _put32(s, dir_at + 4, 264)),
        ("tile size larger than what is left", _put32(s, dir_at + 4 * (nt - 1), int(sizes[-1]) + 16)),
        ("sizes that do not add up", _put32(s, dir_at, int(sizes[0]) - 16)),
        ("16 bytes too many", s + bytes(16)),
    ]
    # one payload word changed so that a lane ends off 2^16: found with the model
    t = nt // 2
    for w in range(8):
        at = int(offs[t]) + 256 + 2 * w
        trial = s[:at] + bytes([s[at] ^ 0x10]) + s[at + 1:]
        if E.decode(trial) is None:
            cases.append(("payload word changed", trial))
            break
    else:
        raise AssertionError("no single-word change is detectable: pick another input")
    # non-zero padding: behind a payload's words, and behind the directory
    for t in range(nt):
        pad = int(sizes[t]) - 256 - 2 * _words_of(s, offs, t)
        if pad >= 2:
            at = int(offs[t + 1]) - 1
            cases.append(("non-zero payload padding", s[:at] + b"\x01" + s[at + 1:]))
            break
    else:
        raise AssertionError("no payload with padding: pick another input")
    if nt % 4:
        cases.append(("non-zero directory padding", s[:fixed - 1] + b"\x01" + s[fixed:]))
    return s, cases


def _table_minus_one(tab):
    f = np.frombuffer(tab, dtype="<u2").copy()
    f[int(np.argmax(f))] -= 1
    return f.tobytes()


def _words_of(s, offs, t):
    """Words the payload of tile t really holds: its size less the states, less trailing zero words is a lower bound; the exact
    count comes from re-encoding, which the caller avoids: padding is what is left after the last non-zero word."""
    body = np.frombuffer(s[int(offs[t]) + 256:int(offs[t + 1])], dtype="<u2")
    nz = np.flatnonzero(body)
    return int(nz[-1]) + 1 if nz.size else 0


def malformed_input():
    n = K * T + 2 * T + 77          # two blocks, 19 tiles (a padded directory), a short last tile
    rng = np.random.default_rng(11)
    return np.minimum(rng.geometric(0.25, n) - 1, 255).astype(np.uint8)


def test_model_rejects_malformed_streams():
    x = malformed_input()
    s, cases = malformed_cases(x)
    assert E.decode(s) == x.tobytes()
    names = [name for name, _ in cases]
    for must in ("payload word changed", "non-zero payload padding", "non-zero directory padding"):
        assert must in names
    for name, bad in cases:
        assert E.decode(bad) is None, name


# -- the library's host arithmetic (no device) ------------------------------------------------------
def test_library_plan_and_bound_against_the_model(pkg):
    L = pkg.lib()
    for n in SIZES + [(1 << 32) + 1, 1 << 36]:
        p = pkg.debug_ec_plan(n)
        assert p == {"T": T, "K": K, "tiles": E.tiles(n), "blocks": E.blocks(E.tiles(n)), "bound": E.bound(n)}
        assert pkg.ec_bound(n) == E.bound(n)
    assert L.bwts_ec_bound(0) == 0 and L.bwts_ec_bound((1 << 36) + 1) == 0
    buf = (ctypes.c_uint64 * 5)()
    assert L.bwts_debug_ec_plan(0, buf) == -1 and L.bwts_debug_ec_plan((1 << 36) + 1, buf) == -1 and L.bwts_debug_ec_plan(5, None) == -1
    lengths = [1, T - 1, T + 1, K * T + 1, 7]
    assert pkg.ec_bound_segments(lengths) == E.bound_segments(lengths)
    got = ctypes.c_uint64(0)
    arr = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    assert L.bwts_ec_bound_segments(None, 1, ctypes.byref(got)) == -1 and L.bwts_ec_bound_segments(arr(5), 0, ctypes.byref(got)) == -1
    assert L.bwts_ec_bound_segments(arr(5, 0, 5), 3, ctypes.byref(got)) == -1 and L.bwts_ec_bound_segments(arr(5), 1, None) == -1
    assert L.bwts_ec_bound_segments(arr(1 << 31, 1 << 31, 1), 3, ctypes.byref(got)) == -5


def test_library_decoded_size_against_the_model(pkg):
    L = pkg.lib()
    x = malformed_input()
    s, cases = malformed_cases(x)
    assert pkg.ec_decoded_size(s) == x.size
    for n in (1, T + 1):
        assert pkg.ec_decoded_size(E.encode(bytes(n))) == n
    got = ctypes.c_uint64(0)
    head = np.frombuffer(s[:16], dtype=np.uint8)
    assert L.bwts_ec_decoded_size(None, len(s), ctypes.byref(got)) == -1 and L.bwts_ec_decoded_size(head.ctypes.data, len(s), None) == -1
    for name, bad in cases:
        if name in ("wrong magic", "wrong params", "cut to 15", "cut inside the directory"):      # what the header and the length alone show
            with pytest.raises(pkg.BwtsError) as e:
                pkg.ec_decoded_size(bad)
            assert e.value.code == pkg.E_FORMAT, name
    big = np.frombuffer(s[:8] + struct.pack("<Q", (1 << 36) + 1), dtype=np.uint8)
    assert L.bwts_ec_decoded_size(big.ctypes.data, 1 << 20, ctypes.byref(got)) == -5
    zero = np.frombuffer(s[:8] + bytes(8), dtype=np.uint8)
    assert L.bwts_ec_decoded_size(zero.ctypes.data, 800, ctypes.byref(got)) == pkg.E_FORMAT
    assert L.bwts_strerror(pkg.E_FORMAT) != b"unknown error" and L.bwts_strerror(pkg.E_SPACE) != b"unknown error"


def test_header_lists_what_the_library_exports(pkg):
    import re
    header = open(os.path.join(ROOT, "include", "bwts_ec.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|uint64_t) (bwts_[a-z0-9_]+)\(", header, flags=re.M)))
    assert declared == sorted(pkg.EC_EXPORTS)
    assert not [s for s in declared if not hasattr(pkg.lib(), s)]


# -- the shared plan and validation header under the sanitizers, as a program of its own -----------------
def test_plan_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ec_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "ec_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.decode().strip().endswith("checks ok")
