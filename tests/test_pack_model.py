"""CPU suite of the packed frame (include/bwts_pack.h): the model (tests/pack_model.py) against zlib and against itself, the committed
version-1 fixtures, the list of malformed frames that the GPU suite shares, the library's host arithmetic against the model, and the
stand-alone host program over the shared frame predicates, built with the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import ec_model as E
import pack_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B0 = P.MIN_BLOCK
ROUND_TRIP_N = [1, 2, 17, 4095, 4096, 4097, 3 * 4096 + 1, 65536 * 4 + 5]
ROUND_TRIP_B = [0, 4096, 4097]


def fixture_input(n, seed):
    """Text-like bytes from integer arithmetic alone (no generator whose stream could change): words of a small vocabulary."""
    words = [b"the", b"block", b"sorting", b"transform", b"of", b"a", b"frame", b"ranks", b"coder", b"and", b"checksum", b"\n"]
    out, x = bytearray(), seed
    while len(out) < n:
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        out += words[(x >> 33) % len(words)] + (b" " if (x >> 40) % 7 else b", ")
    return bytes(out[:n])


FIXTURES = {"pack_v1_one_block.bwz": (fixture_input(3001, 1), 0), "pack_v1_three_blocks.bwz": (fixture_input(2 * B0 + 777, 2), B0)}


# -- CRC arithmetic -------------------------------------------------------------------------------------
def test_crc32_combine_against_zlib():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, (1 << 20) + 5000, dtype=np.uint8).tobytes()
    for la, lb in [(0, 0), (0, 1), (1, 0), (1, 1), (5, 0), (7, 1), (1000, 1 << 20), (1 << 20, 4999), (0, 1 << 20)] + \
            [tuple(int(v) for v in rng.integers(0, 3000, 2)) for _ in range(40)]:
        a, b = data[:la], data[la:la + lb]
        assert P.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
    assert P.xpow8(0) == 0x80000000 and P.gf_mul(0x80000000, 0x12345678) == 0x12345678


# -- the model against itself ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROUND_TRIP_N)
def test_model_round_trip(n):
    x = fixture_input(n, n)
    for B in ROUND_TRIP_B:
        f = P.pack(x, B)
        real_b = n if B == 0 or B >= n else B
        nblk = -(-n // real_b)
        assert len(f) % 16 == 0 and len(f) <= P.bound(n, B)
        assert struct.unpack("<IIQQ", f[:24]) == (P.MAGIC, 1, n, real_b)
        assert P.unpack_size(f) == (n, len(f)) and P.unpack_size(f + bytes(32)) == (n, len(f))
        assert P.unpack(f) == x
        # the streams are what the coder's segment form writes for these lengths
        ranks = b"".join(P.M.forward_fast(P.O.forward(np.frombuffer(x[at:at + real_b], dtype=np.uint8)).tobytes()) for at in range(0, n, real_b))
        assert f[32 + 16 * nblk:] == b"".join(E.encode_segments(ranks, P.lengths(n, real_b)))


def test_model_arguments():
    assert P.block_len(10, 4095) == 10 and P.block_len(5000, 4095) is None and P.block_len(5000, 4096) == 4096
    assert P.block_len(0, 0) is None and P.block_len((1 << 32) + 1, 0) is None and P.block_len(1 << 32, 1 << 33) == 1 << 32
    assert P.bound(5000, 100) == 0 and P.bound(1, 0) == 48 + E.bound(1)
    with pytest.raises(P.PackError) as e:
        P.pack(bytes(5000), 100)
    assert e.value.code == P.E_ARG
    with pytest.raises(P.PackError) as e:
        P.unpack(P.pack(b"abc"), out_cap=2)
    assert e.value.code == P.E_SPACE


def test_committed_fixtures_are_the_models_output():
    for name, (x, B) in FIXTURES.items():
        got = open(os.path.join(GOLDEN, name), "rb").read()
        assert 1024 < len(got) < 16384, name
        assert got == P.pack(x, B), name
        assert P.unpack(got) == x, name
    assert struct.unpack("<QQ", open(os.path.join(GOLDEN, "pack_v1_three_blocks.bwz"), "rb").read()[8:24]) == (2 * B0 + 777, B0)


# -- malformed frames ---------------------------------------------------------------------------------------
def _put(frame, at, fmt, *vals):
    raw = struct.pack(fmt, *vals)
    return frame[:at] + raw + frame[at + len(raw):]


def malformed_input():
    """Three blocks of 4096, 4096 and 100 bytes; the first two differ."""
    return fixture_input(B0, 5) + fixture_input(B0, 6) + fixture_input(100, 7)


def malformed_cases():
    """(name, frame, code): one frame per BWTS_E_FORMAT / BWTS_E_RANGE condition of the header's list, the coder's own refusals, and
    the BWTS_E_CHECKSUM cases; shared with the GPU suite, which must see each refused by the model with that code first."""
    x = malformed_input()
    f = P.pack(x, B0)
    n, B, entries, _ = P.check(f)
    sb = [e[0] for e in entries]
    at = [32 + 16 * 3, 32 + 16 * 3 + sb[0], 32 + 16 * 3 + sb[0] + sb[1]]
    one = P.pack(x[:B0])                                     # a frame of one block
    _s100 = P._stream(np.frombuffer(fixture_input(101, 7), dtype=np.uint8))        # the valid stream of 101 bytes where one of 100 belongs
    _other = P._stream(np.frombuffer(fixture_input(B0, 8), dtype=np.uint8))        # the valid stream of other bytes of a block's length
    F, R, C = P.E_FORMAT, P.E_RANGE, P.E_CHECKSUM
    cases = [
        ("cut to 32 bytes", f[:32], F),
        ("cut to 40 bytes", f[:40], F),
        ("8 bytes too many", f + bytes(8), F),
        ("wrong magic", P.reseal(_put(f, 0, "<I", 0x5A545743)), F),
        ("version 2", P.reseal(_put(f, 4, "<I", 2)), F),
        ("header CRC wrong", _put(f, 28, "<I", struct.unpack("<I", f[28:32])[0] ^ 1), F),
        ("header byte changed, CRC left", _put(f, 9, "<B", f[9] ^ 1), F),
        ("n = 0", P.reseal(_put(f, 8, "<Q", 0)), F),
        ("n = 2^32 + 1", P.reseal(_put(f, 8, "<Q", (1 << 32) + 1)), R),
        ("B = 0", P.reseal(_put(f, 16, "<Q", 0)), F),
        ("B > n", P.reseal(_put(f, 16, "<Q", n + 1)), F),
        ("B = 4095 < n", P.reseal(_put(f, 16, "<Q", 4095)), F),
        ("directory longer than the frame", P.reseal(_put(f, 8, "<Q", 1 << 32)), F),
        ("directory CRC wrong", _reseal_header_only(_put(f, 24, "<I", struct.unpack("<I", f[24:28])[0] ^ 0x100)), F),
        ("directory byte changed, CRC left", _put(f, 32 + 16 + 8, "<B", f[32 + 16 + 8] ^ 1), F),
        ("nonzero reserved word", P.reseal(_put(f, 32 + 16 + 12, "<I", 1)), F),
        ("stream_bytes + 8", P.reseal(_put(f, 32 + 16, "<Q", sb[1] + 8)), F),
        ("stream_bytes = 16", P.reseal(_put(f, 32 + 16, "<Q", 16)), F),
        ("stream_bytes = 2^63", P.reseal(_put(f, 32 + 32, "<Q", 1 << 63)), F),
        ("sizes add up to more", P.reseal(_put(f, 32, "<Q", sb[0] + 16)), F),
        ("16 bytes too many", f + bytes(16), F),
        ("cut by 16", f[:-16], F),
        # what the coder refuses passes through
        ("stream magic changed", _put(f, at[1], "<I", 0x43455743), F),
        ("stream of another length in its place", P.assemble(n, B, [(sb[0], entries[0][1], 0), (sb[1], entries[1][1], 0), (len(_s100), entries[2][1], 0)],
                                                             [f[at[0]:at[1]], f[at[1]:at[2]], _s100]), F),
        ("one block: stream of a longer input", P.assemble(B0 - 1, B0 - 1, [(sb[0], 0, 0)], [f[at[0]:at[1]]]), F),
        ("one block: stream of a shorter input", P.assemble(B0 + 1, B0 + 1, [(sb[0], 0, 0)], [f[at[0]:at[1]]]), F),
        # in bounds, but not the bytes that were packed
        ("directory CRC of a block changed", P.reseal(_put(f, 32 + 8, "<I", entries[0][1] ^ 0x80000000)), C),
        ("two blocks' streams swapped", P.assemble(n, B, [(sb[1], entries[0][1], 0), (sb[0], entries[1][1], 0), (sb[2], entries[2][1], 0)],
                                                   [f[at[1]:at[2]], f[at[0]:at[1]], f[at[2]:]]), C),
        ("a block's stream replaced by another valid one", P.assemble(n, B, [(len(_other), entries[0][1], 0)] + [(s, c, 0) for s, c in entries[1:]],
                                                                      [_other, f[at[1]:]]), C),
        ("one block: CRC changed", P.reseal(_put(one, 32 + 8, "<I", struct.unpack("<I", one[40:44])[0] ^ 1)), C),
    ]
    return x, f, cases


def _reseal_header_only(frame):
    return frame[:28] + struct.pack("<I", zlib.crc32(frame[:28])) + frame[32:]


def test_model_refuses_malformed_frames():
    x, f, cases = malformed_cases()
    assert P.unpack(f) == x
    codes = [c for _, _, c in cases]
    assert codes.count(P.E_CHECKSUM) >= 3 and codes.count(P.E_RANGE) == 1
    for name, bad, code in cases:
        with pytest.raises(P.PackError) as e:
            P.unpack(bad)
        assert e.value.code == code, name


def test_swapped_blocks_decode_cleanly_into_each_others_place():
    x, f, cases = malformed_cases()
    bad = dict((name, fr) for name, fr, _ in cases)["two blocks' streams swapped"]
    n, B, entries, _ = P.check(bad)
    at = 32 + 16 * 3
    first = P.E.decode(bad[at:at + entries[0][0]], want_n=B0)
    assert first is not None
    assert P.O.inverse(np.frombuffer(P.M.inverse_fast(first), dtype=np.uint8)).tobytes() == x[B0:2 * B0]


# -- the library's host arithmetic (no device) ------------------------------------------------------
def test_library_bound_against_the_model(pkg):
    L = pkg.lib()
    for n in ROUND_TRIP_N + [1 << 20, (1 << 32) - 1, 1 << 32]:
        for B in ROUND_TRIP_B + [65536, 1 << 33]:
            assert L.bwts_pack_bound(n, B) == P.bound(n, B), (n, B)
            if P.bound(n, B):
                assert pkg.pack_bound(n, B) == P.bound(n, B)
    assert L.bwts_pack_bound(0, 0) == 0 and L.bwts_pack_bound((1 << 32) + 1, 0) == 0 and L.bwts_pack_bound(5000, 4095) == 0
    assert L.bwts_pack_bound(4000, 100) == 0 and L.bwts_pack_bound(100, 100) == P.bound(100, 0)
    with pytest.raises(pkg.BwtsError):
        pkg.pack_bound(0)


def test_library_unpack_size_against_the_model(pkg):
    L = pkg.lib()
    x, f, cases = malformed_cases()
    assert pkg.unpack_size(f) == (len(x), len(f))
    assert pkg.unpack_size(f + f[:48]) == (len(x), len(f))            # stepping through concatenated frames
    for name, (y, B) in FIXTURES.items():
        g = P.pack(y, B)
        assert pkg.unpack_size(g) == (len(y), len(g))
    n, fb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    a = np.frombuffer(f, dtype=np.uint8)
    assert L.bwts_unpack_size(None, len(f), ctypes.byref(n), ctypes.byref(fb)) == -1
    assert L.bwts_unpack_size(a.ctypes.data, len(f), None, ctypes.byref(fb)) == -1
    assert L.bwts_unpack_size(a.ctypes.data, len(f), ctypes.byref(n), None) == -1
    for name, bad, code in cases:
        try:
            want = P.unpack_size(bad)
        except P.PackError as e:
            with pytest.raises(pkg.BwtsError) as got:
                pkg.unpack_size(bad)
            assert got.value.code == e.code, name
        else:
            assert pkg.unpack_size(bad) == want, name                 # what only the streams or the checksums show


def test_header_lists_what_the_library_exports(pkg):
    header = open(os.path.join(ROOT, "include", "bwts_pack.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|uint64_t) (bwts_[a-z0-9_]+)\(", header, flags=re.M)))
    assert declared == sorted(pkg.PACK_EXPORTS)
    assert not [s for s in declared if not hasattr(pkg.lib(), s)]
    assert not set(pkg.PACK_EXPORTS) & set(pkg.EXPORTS + pkg.MTF_EXPORTS + pkg.EC_EXPORTS + pkg.TEST_EXPORTS)
    assert hasattr(pkg.lib(), "bwts_debug_crc_plan") and "bwts_debug_crc_plan" in pkg.TEST_EXPORTS


def test_strerror_knows_the_checksum_code(pkg):
    assert pkg.E_CHECKSUM == -10 == P.E_CHECKSUM
    msg = pkg.lib().bwts_strerror(-10)
    assert msg != b"unknown error" and b"checksum" in msg.lower()


def test_crc_plan_hook(pkg):
    p = pkg.debug_crc_plan(1)
    T, G = p["T"], p["G"]
    assert p == {"T": T, "G": G, "tiles": 1, "groups": 1} and T % 1024 == 0
    assert 2 * G * T + T + 7 <= 64 << 20                              # the GPU suite's largest size stays small
    for n in (T, T + 1, G * T, G * T + 1, 1 << 36):
        assert pkg.debug_crc_plan(n) == {"T": T, "G": G, "tiles": -(-n // T), "groups": -(-(-(-n // T)) // G)}
    buf = (ctypes.c_uint64 * 4)()
    L = pkg.lib()
    assert L.bwts_debug_crc_plan(0, buf) == -1 and L.bwts_debug_crc_plan((1 << 36) + 1, buf) == -1 and L.bwts_debug_crc_plan(5, None) == -1


# -- the frame predicates under the sanitizers, as a program of its own ---------------------------------------
def test_plan_header_under_sanitizers(tmp_path):
    """tests/pack_plan_check.cc drives the predicates of pack_plan.h over every frame of the list (the answer must be the model's for
    header and directory: 0 where only the streams or the checksums are wrong) and over a valid frame cut at every length below 96."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    x, f, cases = malformed_cases()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as out:
        for name, frame, _ in [("valid", f, 0)] + cases:
            try:
                P.check(frame)
                want = 0
            except P.PackError as e:
                want = e.code
            out.write(struct.pack("<iI", want, len(frame)) + frame)
    exe = str(tmp_path / "pack_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "pack_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, (r.stdout.decode(errors="replace")[-1000:], r.stderr.decode(errors="replace")[-2000:])
    assert r.stdout.decode().strip().endswith("checks ok")
