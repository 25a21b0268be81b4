"""CPU suite of range reads of a packed frame (include/bwts_pack.h, "Ranges"): the model (tests/pack_range_model.py) against the
model's full unpack, what a range read does and does not notice of a damaged frame, the order of the refusals, the library's plan
(host arithmetic, no device) against the model's, and the plan under the sanitizers as a program of its own."""
import functools
import glob
import os
import shutil
import struct
import subprocess

import pytest

import pack_model as P1
import pack_range_model as R
import pack_v2_model as P2
import pack_v3_model as P
from test_pack_model import fixture_input
from test_pack_v3_model import malformed_cases, typed_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B0 = 4096
N6 = 5 * B0 + 3                                     # six blocks, the last of 3 bytes
KINDS = [(1, 0), (2, 0), (3, 2), (3, 4), (3, 8)]    # (version, width)
SHAPES = [(N6, B0), (1, 0), (4097, 0)]              # (n, block_bytes); 0: one block, B = n
BIG = (1 << 64) - 1


def frame_input(version, n):
    return typed_input(n, 11 * n + version) if version == 3 else fixture_input(n, 11 * n + version)


@functools.lru_cache(maxsize=None)
def model_frame(version, width, n, B):
    x = frame_input(version, n)
    f = P1.pack(x, B) if version == 1 else P2.pack(x, B) if version == 2 else P.pack(x, width, B)
    return x, f


def all_frames():
    return [(v, w, n, B) for v, w in KINDS for n, B in SHAPES]


def golden_frames():
    names = sorted(glob.glob(os.path.join(GOLDEN, "pack_*")))
    names = [p for p in names if os.path.isfile(p) and not p.endswith(".py")]
    assert len(names) >= 7
    return [(os.path.basename(p), open(p, "rb").read()) for p in names]


def code_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except P.PackError as e:
        return e.code
    return 0


# -- the model against the model's full unpack -----------------------------------------------------------------------
@pytest.mark.parametrize("version,width", KINDS)
def test_model_against_the_full_unpack(version, width):
    for n, B in SHAPES:
        x, f = model_frame(version, width, n, B)
        assert P.unpack(f) == x
        real_b = B or n
        sets = R.range_sets(n, real_b)
        assert len(sets) == (14 if B else 4 if n == 1 else 6)
        for name, rs in sets:
            got = R.unpack_ranges(f, rs)
            assert got == [x[o:o + b] for o, b in rs], (version, width, n, name)
            p = R.plan(f, rs)
            assert p["out_bytes"] == sum(b for _, b in rs) and p["covered_bytes"] == sum(p["lengths"][b] for b in p["covered"])
            assert len(p["runs"]) == len(p["streams"]) and sum(k for _, k in p["runs"]) == p["blocks"]
            if name == "three runs":
                assert p["runs"] == [(0, 1), (2, 1), (4, 2)]
            if name == "an uncovered block between two ranges":
                assert p["runs"] == [(0, 1), (2, 1)]
            if name == "the last block alone":
                assert p["runs"] == [(5, 1)] and p["covered_bytes"] == 3
            if not B:
                assert p["runs"] == [(0, 1)] and p["covered_bytes"] == n      # a frame of one block is covered whole by any range


# -- only covered blocks are read -------------------------------------------------------------------------------------
def stream_spans(f):
    p = R.plan(f, [(0, 1)])
    return p["stream_at"], p["entries"]


def flip(f, at):
    return f[:at] + bytes([f[at] ^ 0x5A]) + f[at + 1:]


def swapped(version, f, a, b):
    """The frame with the streams and sizes of blocks a < b exchanged, their checksums left where they were: a sound frame."""
    at, entries = stream_spans(f)
    n, B = struct.unpack("<QQ", f[8:24])
    streams = [f[at[k]:at[k + 1]] for k in range(len(entries))]
    streams[a], streams[b] = streams[b], streams[a]
    width = struct.unpack("<I", f[44:48])[0]
    ents = []
    for k, (sb, crc, coded) in enumerate(entries):
        j = b if k == a else a if k == b else k
        ents.append((entries[j][0], crc, width, entries[j][2], 0))
    if version == 1:
        return P1.assemble(n, B, [(e[0], e[1], 0) for e in ents], streams)
    return P2.assemble(n, B, ents, streams, version)


def damage_cases(version, width):
    return damage_cases_of(version, *model_frame(version, width, N6, B0))


def damage_cases_of(version, x, f):
    """(name, frame, ranges, the full unpack's code, the range read's code): ranges inside blocks 1 and 3 of the six-block frame f of x."""
    at, _ = stream_spans(f)
    rs = [(B0 + 5, 20), (3 * B0 + 100, 7)]
    uncovered = flip(f, (at[2] + at[3]) // 2)
    covered = flip(f, (at[3] + at[4]) // 2)
    sw = swapped(version, f, 1, 3)
    full = code_of(P.unpack, covered)
    assert full in (P.E_FORMAT, P.E_CHECKSUM) and code_of(P.unpack, uncovered) in (P.E_FORMAT, P.E_CHECKSUM)
    return x, [("uncovered block damaged", uncovered, rs, code_of(P.unpack, uncovered), 0),
               ("covered block damaged", covered, rs, full, full),
               ("two covered blocks swapped", sw, rs, P.E_CHECKSUM, P.E_CHECKSUM),
               ("two blocks swapped, one covered", sw, [(B0 + 5, 20)], P.E_CHECKSUM, P.E_CHECKSUM),
               ("two blocks swapped, neither covered", sw, [(5, 20), (2 * B0, 1)], P.E_CHECKSUM, 0)]


@pytest.mark.parametrize("version,width", KINDS)
def test_only_covered_blocks_are_read(version, width):
    x, cases = damage_cases(version, width)
    for name, bad, rs, full, ranged in cases:
        assert code_of(P.unpack, bad) == full != 0, name
        assert code_of(R.unpack_ranges, bad, rs) == ranged, name
        if ranged == 0:
            assert R.unpack_ranges(bad, rs) == [x[o:o + b] for o, b in rs], name


# -- the refusals and their order ---------------------------------------------------------------------------------------
def bad_range_cases(n):
    """(name, ranges, out_cap, code) for a valid frame of n bytes."""
    A, G, S = R.E_ARG, R.E_RANGE, R.E_SPACE
    return [("no ranges", [], None, A), ("a range of no bytes", [(0, 1), (5, 0)], None, A), ("no bytes at the end", [(n, 0)], None, A),
            ("no bytes before a range that leaves the input", [(n, 1), (0, 0)], None, A),
            ("one byte too far", [(n - 1, 2)], None, G), ("begins at the end", [(n, 1)], None, G), ("longer than the input", [(0, n + 1)], None, G),
            ("offset + bytes = 2^64 - 1 + 2", [(BIG, 2)], None, G), ("offset + bytes = 2^64", [(BIG, 1)], None, G), ("bytes = 2^64 - 1", [(1, BIG)], None, G),
            ("both 2^63", [(1 << 63, 1 << 63)], None, G), ("leaves the input before the room is judged", [(n - 1, 2)], 0, G),
            ("one byte short", [(0, 10), (3, 10)], 19, S), ("no room", [(0, 1)], 0, S)]


def test_range_arguments_in_order():
    x, f = model_frame(2, 0, N6, B0)
    for name, rs, cap, code in bad_range_cases(len(x)):
        assert code_of(R.unpack_ranges, f, rs, cap) == code, name
        assert code_of(R.plan, f, rs, cap) == code, name
    assert R.unpack_ranges(f, [(0, 10), (3, 10)], 20) == [x[:10], x[3:13]]
    assert code_of(R.check_ranges, 1 << 32, [(0, 1)] * ((1 << 20) + 1)) == R.E_RANGE
    assert code_of(R.check_ranges, 1 << 32, [(0, 1 << 32), (0, 1)]) == R.E_RANGE            # the sum above 2^32
    assert R.check_ranges(1 << 32, [(0, 1 << 32)]) == 1 << 32


def frame_refusal(bad):
    """What header and directory of a frame are refused with, 0 where only the streams or the checksums are wrong."""
    return code_of(P.check, bad)


def test_malformed_frames_give_their_own_codes_whatever_the_ranges():
    x, f, cases = malformed_cases()
    assert R.unpack_ranges(f, [(0, len(x))]) == [x]
    range_lists = [[(0, 1)], [], [(0, 0)], [(BIG, 2)], [(0, 1 << 40)]]
    seen = 0
    for name, bad, code in cases:
        head = frame_refusal(bad)
        for rs in range_lists:
            got = code_of(R.unpack_ranges, bad, rs, 0 if rs == [(0, 1)] and head else None)
            if head:
                assert got == head == code, (name, rs)         # the frame's refusal comes before any range's
                seen += 1
            elif rs != [(0, 1)]:
                assert got == code_of(R.check_ranges, 1, rs), (name, rs)
        if not head:
            # sound header and directory: a read of everything meets what the full unpack meets
            n = struct.unpack("<Q", bad[8:16])[0]
            assert code_of(R.unpack_ranges, bad, [(0, n)]) == code, name
    assert seen >= 5 * 25


# -- the library's plan (host arithmetic, no device) against the model's -------------------------------------------------
def plan_cases():
    """(name, frame, ranges, out_cap): every frame and range set above, the damage cases, the bad ranges, the malformed frames, and
    the committed fixtures with a middle range each."""
    out = []
    for v, w, n, B in all_frames():
        _, f = model_frame(v, w, n, B)
        out += [("v%d w%d n%d: %s" % (v, w, n, name), f, rs, None) for name, rs in R.range_sets(n, B or n)]
    for v, w in KINDS:
        out += [("v%d w%d: %s" % (v, w, name), bad, rs, None) for name, bad, rs, _, _ in damage_cases(v, w)[1]]
    x, f = model_frame(2, 0, N6, B0)
    out += [(name, f, rs, cap) for name, rs, cap, _ in bad_range_cases(len(x))]
    for name, bad, _ in malformed_cases()[2]:
        out += [("malformed: " + name, bad, [(0, 1)], None), ("malformed, no ranges: " + name, bad, [], None)]
    for name, g in golden_frames():
        n = P.check(g)[1]
        out.append(("golden " + name, g, [(n // 3, n // 3 + 1)], None))
    return out


def frame_head(f):
    """Header and directory, which are all the plan reads; all of the frame where those are refused."""
    return f if frame_refusal(f) else f[:32 + (16 if f[4] == 1 else 32) * len(P.lengths(*struct.unpack("<QQ", f[8:24])))]


def model_plan_or_code(f, rs, cap):
    try:
        p = R.plan(f, rs, cap)
    except P.PackError as e:
        return e.code, None
    return 0, {k: p[k] for k in ("blocks", "runs", "covered_bytes", "stream_bytes", "coded_bytes", "out_bytes", "streams", "out")}


def test_library_plan_equals_the_models(pkg):
    cases = plan_cases()
    ok = 0
    for name, f, rs, cap in cases:
        want, p = model_plan_or_code(f, rs, cap)
        head = frame_head(f)
        if want == 0:
            got = pkg.debug_unpack_ranges_plan(head, rs, cap, in_bytes=len(f))
            assert got.pop("T") == R.T, name
            assert got == p, name
            ok += 1
        else:
            with pytest.raises(pkg.BwtsError) as e:
                pkg.debug_unpack_ranges_plan(head, rs, cap, in_bytes=len(f))
            assert e.value.code == want, name
    assert ok >= 100 and len(cases) - ok >= 60


def test_plan_hook_arguments(pkg):
    L = pkg.lib()
    _, f = model_frame(1, 0, N6, B0)
    assert L.bwts_debug_unpack_ranges_plan(None, len(f), None, 0, 0, None, None, 0) == -1
    assert "bwts_debug_unpack_ranges_plan" in pkg.TEST_EXPORTS and "bwts_unpack_ranges" in pkg.PACK_EXPORTS
    p = pkg.debug_unpack_ranges_plan(f, [(0, 1)])
    assert p["T"] == R.T and p["T"] % 16 == 0 and p["runs"] == [(0, 1)]


# -- the plan under the sanitizers, as a program of its own ---------------------------------------------------------------
def write_cases_file(path):
    """plan_cases() with the model's answers, in the layout that tests/pack_range_check.cc reads (tests/members_plan_check.cc too)."""
    with open(path, "wb") as out:
        for name, f, rs, cap in plan_cases():
            want, p = model_plan_or_code(f, rs, cap)
            words = []
            if want == 0:
                words = [p["blocks"], len(p["runs"]), p["covered_bytes"], p["stream_bytes"], p["coded_bytes"], p["out_bytes"]]
                words += [v for r in p["runs"] for v in r] + [v for s in p["streams"] for v in s] + [v for o in p["out"] for v in o]
            head = frame_head(f)
            out.write(struct.pack("<iIQQII", want, len(head), len(f), BIG if cap is None else cap, len(rs), len(words)) + head)
            out.write(b"".join(struct.pack("<QQ", o, b) for o, b in rs) + b"".join(struct.pack("<Q", v) for v in words))


def test_plan_under_sanitizers(tmp_path):
    """tests/pack_range_check.cc drives pack_ranges_check and the range plan over every case above, each from heap blocks of exactly
    the header's, directory's and ranges' length, and over a valid directory with hostile ranges: overflowing sums, 2^20 one-byte
    ranges in one block."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path / "cases.bin")
    write_cases_file(path)
    exe = str(tmp_path / "pack_range_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "pack_range_check.cc"), "-o", exe])
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, (r.stdout.decode(errors="replace")[-1000:], r.stderr.decode(errors="replace")[-2000:])
    assert r.stdout.decode().strip().endswith("checks ok")
