"""CPU suite of the delta filter (include/bwts_delta.h): the model (tests/delta_model.py) against the literal loop of the definition and
against vectors written by hand, its round trips in both orders, the segment form, the library's export list, and the stand-alone host
program over the shared plan header (and the version-2 predicates of the member frame), built with the address and undefined-behaviour
sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import delta_model as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENT_LENGTHS = [1, 3, 7, 8, 9, 4096, 4097, 65541, 2, 16385]


def lengths_for(w):
    return [1, w - 1, w, w + 1, 16 * w - 1, 4095, 4096, 4097, 4096 * w + 1, 70001]


def literal_encode(x, w):
    """d_0 = a_0, d_i = a_i - a_{i-1}; z_i = (d_i << 1) xor (d_i >> (8w - 1), arithmetically): the header's lines, as a loop over Python
    integers, the arithmetic shift spelled out on a signed value."""
    L, q, m = len(x), len(x) // w, (1 << (8 * w)) - 1
    out, prev = bytearray(x), 0
    for i in range(q):
        a = int.from_bytes(x[i * w:(i + 1) * w], "little")
        d = (a - prev) & m
        signed = d - (1 << (8 * w)) if d >> (8 * w - 1) else d
        out[i * w:(i + 1) * w] = (((signed << 1) ^ (signed >> (8 * w - 1))) & m).to_bytes(w, "little")
        prev = a
    assert out[q * w:] == x[q * w:] and len(out) == L
    return bytes(out)


def some_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("w", D.WIDTHS)
def test_encode_is_the_definition_and_decode_its_inverse(w):
    for L in lengths_for(w):
        for x in (some_bytes(L, L + w), np.full(L, 0xFF, dtype=np.uint8), np.zeros(L, dtype=np.uint8)):
            y = D.encode(x, w)
            assert y.dtype == np.uint8 and y.size == L
            assert y.tobytes() == literal_encode(x.tobytes(), w), (w, L)
            assert np.array_equal(D.decode(y, w), x), (w, L)
            # every byte string is a valid input of the decoder too, and encode takes it back
            assert np.array_equal(D.encode(D.decode(x, w), w), x), (w, L)
            if L < w:
                assert np.array_equal(y, x)
            assert np.array_equal(y[L // w * w:], x[L // w * w:])


def test_vectors_by_hand():
    h = bytes.fromhex
    # width 1: 5, 3 (-2), 3 (0), 4 (+1), 0x84 (-128: the largest code)
    assert D.encode(h("0503030484"), 1).tobytes() == h("0a030002ff")
    # wraparound at width 1: 0xFF then 0x00 is +1, 0x00 then 0xFF is -1
    assert D.encode(h("ff00ff"), 1).tobytes() == h("010201")
    # width 2, little-endian: 0x0100, 0x00FF (-1), 0x8000 (+0x7F01), 0x0000 (-0x8000: 0x8000 is its own negative, the largest code)
    assert D.encode(h("0001ff0000800000"), 2).tobytes() == h("00020100" "02fe" "ffff")
    # width 4: the first element is zigzagged too: 0x80000000 becomes 0xFFFFFFFF, then +1, then a tail of three bytes
    assert D.encode(h("00000080010000806162" "63"), 4).tobytes() == h("ffffffff02000000" "616263")
    # width 8: 0x80 00 ... 00 alone, and a wrap from 2^64 - 1 to 0
    assert D.encode(h("0000000000000080"), 8).tobytes() == h("ffffffffffffffff")
    assert D.encode(h("ffffffffffffffff0000000000000000"), 8).tobytes() == h("01000000000000000200000000000000")
    # all 0xFF: the first element is -1, every other difference 0
    for w in D.WIDTHS:
        assert D.encode(b"\xff" * (3 * w + w - 1), w).tobytes() == b"\x01" + bytes(3 * w - 1) + b"\xff" * (w - 1)
    # shorter than an element: the identity
    assert D.encode(b"abc", 4).tobytes() == b"abc" and D.decode(b"abcdefg", 8).tobytes() == b"abcdefg"
    for vec, w in ((h("0a030002ff"), 1), (h("0002010002feffff"), 2), (h("ffffffff02000000616263"), 4), (h("ffffffffffffffff"), 8)):
        assert D.encode(D.decode(vec, w), w).tobytes() == vec
    assert D.decode(h("0a030002ff"), 1).tobytes() == h("0503030484")
    assert [D.zigzag(d, 1) for d in (0, -1, 1, -2, 2, 127, -128)] == [0, 1, 2, 3, 4, 254, 255]
    assert [D.unzigzag(z, 2) for z in (0, 1, 2, 3, 0xFFFE, 0xFFFF)] == [0, 0xFFFF, 1, 0xFFFE, 0x7FFF, 0x8000]


def test_widths():
    for w in (0, 3, 5, 16, -2):
        with pytest.raises(ValueError):
            D.encode(b"abcdefgh", w)
        with pytest.raises(ValueError):
            D.decode(b"abcdefgh", w)
    with pytest.raises(ValueError):
        D.encode_segments(b"abcdefgh", [8], [4], [2])


def test_segment_form():
    widths = [(1, 2, 4, 8)[k % 4] for k in range(len(SEGMENT_LENGTHS))]
    filters = [(1, 1, 0)[k % 3] for k in range(len(SEGMENT_LENGTHS))]
    x = some_bytes(sum(SEGMENT_LENGTHS), 3)
    y = D.encode_segments(x, SEGMENT_LENGTHS, widths, filters)
    at = 0
    for ln, w, f in zip(SEGMENT_LENGTHS, widths, filters):
        want = D.encode(x[at:at + ln], w) if f else x[at:at + ln]
        assert np.array_equal(y[at:at + ln], want), (w, ln, f)
        at += ln
    assert np.array_equal(D.decode_segments(y, SEGMENT_LENGTHS, widths, filters), x)
    assert np.array_equal(D.encode_segments(x, [x.size], [4], [1]), D.encode(x, 4))
    assert np.array_equal(D.encode_segments(x, [x.size], [4], [0]), x)
    assert D.tiles(4096 * 4 + 1, 4, 1) == 2 and D.tiles(4096 * 4 + 1, 4, 0) == 1 and D.tiles(32769, 1, 0) == 2 and D.tiles(4097, 1, 1) == 2


# -- the library's export list (no device) ---------------------------------------------------------------
def test_header_declares_what_the_library_exports(pkg):
    header = open(os.path.join(ROOT, "include", "bwts_delta.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|uint64_t) (bwts_[a-z0-9_]+)\(", header, flags=re.M)))
    assert declared == sorted(pkg.DELTA_EXPORTS) and len(declared) == 6
    assert not [s for s in declared if not hasattr(pkg.lib(), s)]
    assert not set(pkg.DELTA_EXPORTS) & set(pkg.EXPORTS + pkg.MTF_EXPORTS + pkg.EC_EXPORTS + pkg.ZRL_EXPORTS + pkg.PLANES_EXPORTS + pkg.PACK_EXPORTS
                                            + pkg.MEMBERS_EXPORTS + pkg.TEST_EXPORTS)
    assert re.search(r"#define BWTS_FILTER_NONE 0u", header) and re.search(r"#define BWTS_FILTER_DELTA 1u", header)
    assert (pkg.FILTER_NONE, pkg.FILTER_DELTA) == (D.FILTER_NONE, D.FILTER_DELTA)


# -- the shared plan header and the version-2 member predicates under the sanitizers, as a program of its own -----------------
def test_plan_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "delta_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "delta_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.decode().strip().endswith("checks ok")
