"""CPU suite of the member frame (include/bwts_members.h): the model (tests/pack_members_model.py) round trips, every refusal of the
header's list in its order, the range plans across member boundaries, the committed fixtures, the library's host arithmetic
(no device) against the model, and the predicates and the plan under the sanitizers as a program of its own."""
import os
import shutil
import struct
import subprocess

import pytest

import members_cases as C
import pack_members_model as MM
import pack_v2_model as P2
import pack_v3_model as P3
from test_pack_model import _put, fixture_input
from test_pack_range_model import write_cases_file as write_bwtz_cases_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIG = (1 << 64) - 1


def code_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except MM.PackError as e:
        return e.code
    return 0


# -- round trips -----------------------------------------------------------------------------------------------------------
def test_round_trip_of_the_member_set():
    members, widths = C.member_set()
    f = C.member_frame()
    assert MM.unpack(f) == b"".join(members)
    assert MM.frame_members(f) == ([len(m) for m in members], widths)
    assert MM.unpack_size(f) == (sum(C.LENGTHS), len(f)) and MM.unpack_size(f + bytes(48)) == (sum(C.LENGTHS), len(f))
    assert len(f) <= MM.bound(C.LENGTHS) and len(f) % 16 == 0
    magic, version, n, count = struct.unpack("<IIQQ", f[:24])
    assert (magic, version, n, count) == (0x4D545742, 1, sum(C.LENGTHS), len(members)) and f[:4] == b"BWTM"
    # the split pays where it should: the float32 members at width 4 and 8 against the same members unsplit
    plain = MM.pack(members, None)
    assert MM.unpack(plain) == b"".join(members) and MM.frame_members(plain)[1] == [1] * len(members)
    k = C.LENGTHS.index(16385)
    assert widths[k] == 4 and k % 3 == 1 and MM.check(f)[1][k][0] < 0.8 * MM.check(plain)[1][k][0]


def test_small_shapes_and_every_width():
    for ln in (1, 2, 3, 7, 8, 9, 17):
        for w in MM.WIDTHS:
            x = fixture_input(ln, ln + w)
            f = MM.pack([x], [w])
            assert MM.unpack(f) == x and len(f) == 64 + MM.check(f)[1][0][0] and MM.frame_members(f) == ([ln], [w])
    # widths None: no split anywhere, and the streams are those of the members alone
    a, b = fixture_input(5000, 1), fixture_input(4097, 2)
    f = MM.pack([a, b])
    assert MM.unpack(f) == a + b and MM.frame_members(f) == ([5000, 4097], [1, 1])
    fa, fb = MM.pack([a]), MM.pack([b])
    assert f[96:] == fa[64:] + fb[64:]


def test_members_of_one_length_at_width_1_are_version_2s_streams():
    """Members of width 1 and one length 4096 make the streams of the version-2 "BWTZ" frame at B = 4096 of the same bytes; header,
    width word and length word alone differ."""
    x = fixture_input(3 * 4096, 21)
    f = MM.pack([x[k:k + 4096] for k in range(0, len(x), 4096)])
    v2 = P2.pack(x, 4096)
    fixed = 32 + 32 * 3
    assert f[fixed:] == v2[fixed:] and len(f) == len(v2)
    for k in range(3):
        e, e2 = f[32 + 32 * k:64 + 32 * k], v2[32 + 32 * k:64 + 32 * k]
        assert e[:12] == e2[:12] and e[16:24] == e2[16:24]
        assert struct.unpack("<I", e[12:16])[0] == 1 and struct.unpack("<Q", e[24:32])[0] == 4096 and e2[12:16] == bytes(4) and e2[24:32] == bytes(8)
    assert f[8:16] == v2[8:16] and struct.unpack("<Q", f[16:24])[0] == 3


def test_arguments():
    x = bytes(10)
    for members, widths, code in (([], None, MM.E_ARG), ([x, b""], None, MM.E_ARG), ([x], [3], MM.E_ARG), ([x], [0], MM.E_ARG), ([x], [16], MM.E_ARG),
                                  ([x, x], [2], MM.E_ARG)):
        assert code_of(MM.pack, members, widths) == code, (members, widths)
    assert code_of(MM.check_args, [1] * ((1 << 20) + 1), None) == MM.E_RANGE
    assert code_of(MM.check_args, [1 << 32, 1], None) == MM.E_RANGE and MM.check_args([(1 << 32) - 1, 1], [8, 1]) == ([8, 1], 1 << 32)
    assert MM.bound([]) == 0 and MM.bound([4, 0]) == 0 and MM.bound([1 << 32, 1]) == 0
    assert MM.bound([5, 4096]) == 32 + 64 + sum(MM.E.bound(v) for v in (5, 4096))
    assert code_of(MM.unpack, MM.pack([b"abc"], [2]), out_cap=2) == MM.E_SPACE


def test_committed_fixtures_are_the_models_output():
    for name, (members, widths) in C.fixtures().items():
        got = open(os.path.join(GOLDEN, name), "rb").read()
        assert 512 < len(got) < 16384, name
        assert got == MM.pack(members, widths), name
        assert MM.unpack(got) == b"".join(members) and MM.unpack_members(got, list(range(len(members)))) == members, name


# -- refusals ---------------------------------------------------------------------------------------------------------------
def test_model_refuses_malformed_frames_in_the_headers_order():
    x, f, cases = C.malformed_cases()
    assert MM.unpack(f) == x
    codes = [c for _, _, c in cases]
    assert codes.count(MM.E_CHECKSUM) >= 6 and codes.count(MM.E_RANGE) == 2 and len(cases) >= 40
    for name, bad, code in cases:
        assert code_of(MM.unpack, bad) == code, name
        # the range read and the member read judge the frame first, with the same code; the stages' and the checksums' cases pass the frame checks
        first = C.frame_code(name, code)
        assert code_of(MM.plan, bad, [(0, 1)]) == first, name
        assert code_of(MM.index_ranges, bad, [0]) == first, name
        # ... and so does frame_members; unpack_size lets a frame end early, and nothing else
        assert code_of(MM.frame_members, bad) == first, name
        if name not in ("16 bytes too many",):
            assert code_of(MM.unpack_size, bad) == first, name
    assert MM.unpack_size(f + bytes(16)) == (len(x), len(f))


def test_a_later_check_does_not_hide_an_earlier_one():
    """Frames that are wrong twice: the earlier check of the list decides."""
    x, f, _ = C.malformed_cases()
    n = len(x)
    with pytest.raises(MM.PackError) as e:
        MM.check(_put(f, 8, "<Q", (1 << 32) + 1)[:48])                      # length, before the header CRC and n
    assert e.value.code == MM.E_FORMAT and "length" in str(e.value)
    with pytest.raises(MM.PackError) as e:
        MM.check(_put(_put(f, 8, "<Q", (1 << 32) + 1), 0, "<I", 0x5A545742))   # magic, before n
    assert e.value.code == MM.E_FORMAT and "magic" in str(e.value)
    with pytest.raises(MM.PackError) as e:
        MM.check(MM.reseal(_put(_put(f, 8, "<Q", (1 << 32) + 1), 16, "<Q", 0)))  # n > 2^32, before count = 0
    assert e.value.code == MM.E_RANGE
    with pytest.raises(MM.PackError) as e:
        MM.check(MM.reseal(_put(_put(f, 8, "<Q", 0), 16, "<Q", (1 << 20) + 1)))   # n = 0, before count > 2^20
    assert e.value.code == MM.E_FORMAT and "n = 0" in str(e.value)
    with pytest.raises(MM.PackError) as e:
        MM.check(MM.reseal(_put(f, 16, "<Q", (1 << 20) + 1)))                # count > n comes before count > 2^20
    assert e.value.code == MM.E_FORMAT and n < (1 << 20)
    # a frame of the other magic goes to its own model, and a member read of it is refused
    v3 = P3.pack(x[:8192], 4, 4096)
    assert MM.unpack(v3) == x[:8192] and MM.unpack_ranges(v3, [(4090, 10)]) == [x[4090:4100]]
    assert code_of(MM.frame_members, v3) == MM.E_FORMAT and code_of(MM.unpack_members, v3, [0]) == MM.E_FORMAT


# -- ranges and members -------------------------------------------------------------------------------------------------------
def test_range_plans_across_member_boundaries():
    members, _ = C.member_set()
    x, f = b"".join(members), C.member_frame()
    off = MM.plan(f, [(0, 1)])["offsets"]
    sets = C.range_sets()
    assert len(sets) == 10
    for name, rs in sets:
        p = MM.plan(f, rs)
        assert MM.unpack_ranges(f, rs) == [x[o:o + b] for o, b in rs], name
        assert p["out_bytes"] == sum(b for _, b in rs) and p["covered_bytes"] == sum(C.LENGTHS[b] for b in p["covered"])
        assert len(p["runs"]) == len(p["streams"]) and sum(k for _, k in p["runs"]) == p["blocks"]
        for o, b in rs:
            for at in (o, o + b - 1):
                k = [j for j in p["covered"] if off[j] <= at < off[j + 1]]
                assert len(k) == 1, (name, at)
        want = {"first byte": [(0, 1)], "last byte": [(12, 1)], "within one member": [(11, 1)], "one member exactly": [(8, 1)],
                "across two members": [(7, 2)], "straddles a seam by a byte each side": [(10, 2)],
                "the short members at the front, each by a byte": [(0, 5)], "an uncovered member between two ranges": [(5, 1), (7, 1)],
                "descending, overlapping, a repeat": [(2, 3), (6, 2), (10, 1)], "whole input": [(0, 13)]}[name]
        assert p["runs"] == want, (name, p["runs"])
    # the codes of the ranges come behind the frame's
    n = len(x)
    for rs, cap, code in ((None, None, MM.E_ARG), ([], None, MM.E_ARG), ([(0, 0)], None, MM.E_ARG), ([(n, 1)], None, MM.E_RANGE), ([(n - 1, 2)], None, MM.E_RANGE),
                          ([(BIG, 2)], None, MM.E_RANGE), ([(0, 10), (5, 10)], 19, MM.E_SPACE)):
        assert code_of(MM.plan, f, rs, cap) == code, (rs, cap)


def test_unpack_members():
    members, _ = C.member_set()
    f = C.member_frame()
    perm = [12, 0, 5, 7, 5, 3]
    assert MM.unpack_members(f, perm) == [members[k] for k in perm]
    assert MM.unpack_members(f, [9]) == [members[9]]
    p = MM.plan(f, MM.index_ranges(f, perm))
    assert p["covered"] == [0, 3, 5, 7, 12] and p["covered_bytes"] == sum(C.LENGTHS[k] for k in (0, 3, 5, 7, 12))      # a member is decoded once
    for idx, cap, code in ((None, None, MM.E_ARG), ([], None, MM.E_ARG), ([13], None, MM.E_RANGE), ([0, BIG], None, MM.E_RANGE), ([1, 1], 3, MM.E_SPACE)):
        assert code_of(MM.unpack_members, f, idx, cap) == code, (idx, cap)
    # damage in a member that is not asked for goes unnoticed; in one that is, it shows
    _, entries, _ = MM.check(f)
    at = MM._stream_at(entries)
    bad = _put(f, (at[10] + at[11]) // 2, "<B", f[(at[10] + at[11]) // 2] ^ 0x5A)
    assert MM.unpack_members(bad, [9, 11]) == [members[9], members[11]]
    assert code_of(MM.unpack_members, bad, [10]) in (MM.E_FORMAT, MM.E_CHECKSUM) and code_of(MM.unpack, bad) in (MM.E_FORMAT, MM.E_CHECKSUM)


def test_mixed_width_split_model():
    members, widths = C.member_set()
    x = b"".join(members)
    y = MM.split_segments(x, C.LENGTHS, widths)
    assert MM.join_segments(y, C.LENGTHS, widths) == x and len(y) == len(x)
    at = 0
    for m, w in zip(members, widths):
        assert y[at:at + len(m)] == MM.split(m, w).tobytes()
        at += len(m)
    assert [MM.tiles(ln, w) for ln, w in ((1, 1), (32768, 1), (32769, 1), (8193, 2), (8192, 2), (32775, 8), (65537, 8))] == [1, 1, 2, 2, 1, 2, 3]


# -- the library's host arithmetic (no device) ---------------------------------------------------------------------------------
def plan_cases():
    """(name, frame, ranges, out_cap): the valid small frame first, every malformed frame, the range sets on the member set's frame, and
    range refusals."""
    x, f, cases = C.malformed_cases()
    out = [("valid", f, [(0, 1)], None), ("valid, all", f, [(0, len(x))], None), ("valid, a seam", f, [(4090, 10), (8292, 9), (8191, 2)], None)]
    out += [(name, bad, [(0, 1)], None) for name, bad, _ in cases]
    big = C.member_frame()
    out += [(name, big, rs, None) for name, rs in C.range_sets()]
    n = sum(C.LENGTHS)
    out += [("no ranges", big, [], None), ("a range of no bytes", big, [(5, 0)], None), ("a range leaves the input", big, [(n - 1, 2)], None),
            ("offset + bytes wraps", big, [(BIG, 2)], None), ("sum above out_cap", big, [(0, 10), (5, 10)], 19), ("sum at out_cap", big, [(0, 10), (5, 10)], 20)]
    return out


def frame_head(f):
    """Header and directory of a frame, all of it where there is no telling."""
    try:
        _, entries, _ = MM.check(f)
    except MM.PackError:
        return f
    return f[:32 + 32 * len(entries)]


def model_plan_or_code(f, rs, cap):
    try:
        return 0, MM.plan(f, rs, cap)
    except MM.PackError as e:
        return e.code, None


def test_library_host_arithmetic_against_the_model(pkg):
    assert set(pkg.MEMBERS_EXPORTS) >= {"bwts_pack_members_device", "bwts_unpack_members_device", "bwts_frame_members", "bwts_planes_split_segments_w_device"}
    for name, f, rs, cap in plan_cases():
        want, p = model_plan_or_code(f, rs, cap)
        try:
            got = pkg.debug_unpack_ranges_plan(f, rs, out_cap=cap)
            code = 0
        except pkg.BwtsError as e:
            code = e.code
        assert code == want, (name, code, want)
        if want == 0:
            for key in ("blocks", "runs", "covered_bytes", "stream_bytes", "coded_bytes", "out_bytes", "streams", "out"):
                assert got[key] == p[key], (name, key)
    x, f, cases = C.malformed_cases()
    assert pkg.frame_members(f) == (C.SMALL_LENGTHS, C.SMALL_WIDTHS) and pkg.unpack_size(f) == (len(x), len(f))
    assert pkg.unpack_size(f + bytes(32)) == (len(x), len(f))
    for name, bad, code in cases:
        first = C.frame_code(name, code)
        for fn in (pkg.frame_members, pkg.unpack_size):
            if fn is pkg.unpack_size and name == "16 bytes too many":
                continue
            try:
                fn(bad)
                got = 0
            except pkg.BwtsError as e:
                got = e.code
            assert got == first, (name, fn.__name__, got, first)
    big = C.member_frame()
    assert pkg.frame_members(big) == (C.LENGTHS, C.WIDTHS)
    assert pkg.pack_members_bound(C.LENGTHS) == MM.bound(C.LENGTHS) and pkg.pack_members_bound([5]) == MM.bound([5])
    for ls, code in (([], -1), ([4, 0], -1), ([1 << 32, 1], -5), ([1] * ((1 << 20) + 1), -5)):
        with pytest.raises(pkg.BwtsError) as e:
            pkg.pack_members_bound(ls)
        assert e.value.code == code, ls
    # a "BWTZ" frame has no members
    with pytest.raises(pkg.BwtsError) as e:
        pkg.frame_members(P3.pack(x[:8192], 4, 4096))
    assert e.value.code == MM.E_FORMAT


# -- the predicates and the plan under the sanitizers, as a program of its own ---------------------------------------------------
def test_plan_under_sanitizers(tmp_path):
    """tests/members_plan_check.cc drives the header and directory predicates and the range plan of members_plan.h over every case
    above, each from heap blocks of exactly the header's, directory's and ranges' length, over the valid frame cut at every length
    below 128, and over a valid directory with hostile ranges and indices.  It also plans every "BWTZ" case of test_pack_range_model
    twice, by division by B and by bisection of the same blocks' offsets, and holds the two plans against each other."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    path = str(tmp_path / "cases.bin")
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
    bwtz = str(tmp_path / "bwtz_cases.bin")
    write_bwtz_cases_file(bwtz)
    exe = str(tmp_path / "members_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "members_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe, path, bwtz], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, (r.stdout.decode(errors="replace")[-1000:], r.stderr.decode(errors="replace")[-2000:])
    assert r.stdout.decode().strip().endswith("checks ok")
