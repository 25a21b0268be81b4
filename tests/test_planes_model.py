"""CPU suite of the byte-plane split (include/bwts_planes.h): the model (tests/planes_model.py) against the literal double loop of the
definition, its round trips, the segment form, the library's host arithmetic and export list, and the stand-alone host program over
the shared plan header (and the version-3 frame predicates), built with the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import planes_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENT_LENGTHS = [1, 3, 7, 8, 9, 4096, 4097, 65541, 2, 16385]


def lengths_for(w):
    return [1, w - 1, w, w + 1, 16 * w - 1, 4095, 4096, 4097, 70001]


def literal_split(x, w):
    """out[k q + i] = in[i w + k]; out[q w + j] = in[q w + j]: the header's two lines, as loops."""
    L = len(x)
    q = L // w
    out = bytearray(L)
    for k in range(w):
        for i in range(q):
            out[k * q + i] = x[i * w + k]
    for j in range(q * w, L):
        out[j] = x[j]
    return bytes(out)


def some_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("w", S.WIDTHS)
def test_split_is_the_definition_and_join_its_inverse(w):
    for L in lengths_for(w):
        x = some_bytes(L, L + w)
        y = S.split(x, w)
        assert y.dtype == np.uint8 and y.size == L
        assert y.tobytes() == literal_split(x.tobytes(), w), (w, L)
        assert np.array_equal(S.join(y, w), x), (w, L)
        if L < w:
            assert np.array_equal(y, x)
        # the tail stays where it is; plane k is byte k of every element
        q = L // w
        assert np.array_equal(y[q * w:], x[q * w:])
        for k in range(w):
            assert np.array_equal(y[k * q:(k + 1) * q], x[k:q * w:w])


def test_widths():
    for w in (0, 1, 3, 5, 16, -2):
        with pytest.raises(ValueError):
            S.split(b"abcdefgh", w)
        with pytest.raises(ValueError):
            S.join(b"abcdefgh", w)
    assert S.split(b"abcdefgh", 2).tobytes() == b"acegbdfh" and S.split(b"abcdefghi", 4).tobytes() == b"aebfcgdhi"
    assert S.join(b"acegbdfh", 2).tobytes() == b"abcdefgh"


@pytest.mark.parametrize("w", S.WIDTHS)
def test_segment_form(w):
    x = some_bytes(sum(SEGMENT_LENGTHS), w)
    y = S.split_segments(x, SEGMENT_LENGTHS, w)
    at = 0
    for ln in SEGMENT_LENGTHS:
        assert np.array_equal(y[at:at + ln], S.split(x[at:at + ln], w)), (w, ln)
        at += ln
    assert np.array_equal(S.join_segments(y, SEGMENT_LENGTHS, w), x)
    assert np.array_equal(S.split_segments(x, [x.size], w), S.split(x, w))


# -- the library's host arithmetic and export list (no device) ---------------------------------------------
def test_library_plan_against_the_model(pkg):
    for w in S.WIDTHS:
        T = S.E * w
        for n in lengths_for(w) + [T - 1, T, T + 1, 2 * T + w + 1, (1 << 20) + 5, (1 << 32) + (1 << 20) + 3, 1 << 36]:
            assert pkg.debug_planes_plan(n, w) == S.plan(n, w), (n, w)
    for n, w in ((0, 4), ((1 << 36) + 1, 4), (100, 0), (100, 1), (100, 3), (100, 16)):
        with pytest.raises(pkg.BwtsError):
            pkg.debug_planes_plan(n, w)


def test_header_declares_what_the_library_exports(pkg):
    header = open(os.path.join(ROOT, "include", "bwts_planes.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|uint64_t) (bwts_[a-z0-9_]+)\(", header, flags=re.M)))
    assert declared == sorted(pkg.PLANES_EXPORTS)
    assert not [s for s in declared if not hasattr(pkg.lib(), s)]
    assert not set(pkg.PLANES_EXPORTS) & set(pkg.EXPORTS + pkg.MTF_EXPORTS + pkg.EC_EXPORTS + pkg.ZRL_EXPORTS + pkg.PACK_EXPORTS + pkg.TEST_EXPORTS)
    assert hasattr(pkg.lib(), "bwts_debug_planes_plan") and "bwts_debug_planes_plan" in pkg.TEST_EXPORTS


# -- the shared plan header and the version-3 frame predicates under the sanitizers, as a program of its own -----------------
def test_plan_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "planes_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "planes_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.decode().strip().endswith("checks ok")
