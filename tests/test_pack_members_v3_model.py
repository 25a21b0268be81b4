"""CPU suite of version 3 of the member frame (include/bwts_members.h): the model (tests/pack_members_v3_model.py) round trips, a pack
without a method is the frame of the earlier versions, every refusal that version 3 adds, the golden frame, the library's host
arithmetic against the model, the plan header under the sanitizers, and the size pin of the direct method."""
import os
import shutil
import struct
import subprocess

import members_cases as C
import members_v2_cases as C2
import members_v3_cases as C3
import pack_members_model as MM
import pack_members_v2_model as M2
import pack_members_v3_model as M3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, CK = MM.E_FORMAT, MM.E_CHECKSUM


def code_of(fn, *args):
    try:
        fn(*args)
        return 0
    except MM.PackError as e:
        return e.code


def test_cut_rule_and_bound():
    assert M3.segments(2 * 8192 - 1, 2) == [16383] and M3.segments(2 * 8192, 2) == [8192, 8192] and M3.segments(2 * 8192 + 1, 2) == [8192, 8193]
    assert M3.segments(8 * 8192 + 7, 8) == [8192] * 7 + [8199] and M3.segments(8 * 8192 - 1, 8) == [65535]
    assert M3.segments(1 << 20, 1) == [1 << 20] and M3.segments(3, 4) == [3]
    for ln, w in ((1, 8), (16384, 2), (16385, 2), (70001, 4), (65536, 8)):
        assert sum(M3.segments(ln, w)) == ln
    ls, ws, ms = [16385, 100, 32768, 9], [2, 4, 4, 8], [1, 1, 1, 0]
    assert M3.ext_words(ls, ws, ms) == 6 and M3.ext_words(ls, ws, [1, 1, 0, 0]) == 2 and M3.ext_words(ls, ws, [0] * 4) == 0
    want = 32 + 32 * 4 + 48 + sum(M3.E.bound(s) for s in (8192, 8193, 100, 8192, 8192, 8192, 8192, 9))
    assert M3.bound(ls, ws, ms) == want and M3.bound(ls, ws, None) == MM.bound(ls) and M3.bound(ls, ws, [0, 2, 0, 0]) == 0
    for args, code in ((([4], [4], None, [2]), MM.E_ARG), (([4], [4], None, [1, 0]), MM.E_ARG), (([4, 0], None, None, [1, 1]), MM.E_ARG),
                       (([1 << 32, 1], None, None, [1, 1]), MM.E_RANGE)):
        assert code_of(M3.check_args, *args) == code, args


def test_a_pack_without_a_method_is_the_earlier_frame():
    members, widths = C.small_set()
    assert M3.pack(members, widths) == MM.pack(members, widths) and M3.pack(members, widths, None, [0] * 4) == MM.pack(members, widths)
    m2, w2, f2 = C2.small_set()
    want = M2.pack(m2, w2, f2)
    assert M3.pack(m2, w2, f2) == want and M3.pack(m2, w2, f2, [0] * 4) == want and M3.version_of(want) == 2
    # every reader takes the earlier versions
    assert M3.unpack(want) == b"".join(m2) and M3.frame_members_m(want) == (C.SMALL_LENGTHS, C.SMALL_WIDTHS, C2.SMALL_FILTERS, [0] * 4)
    assert M3.unpack_members(want, [3, 0]) == [m2[3], m2[0]]


def test_round_trips():
    specs = [
        [(2 * 8192 - 1, 2, 0, 1)], [(2 * 8192, 2, 0, 1)], [(4 * 8192 + 3, 4, 0, 1)], [(5000, 1, 0, 1)], [(3, 4, 0, 1)], [(8 * 8192 + 7, 8, 1, 1)],
        [(5000, 2, 0, 1), (4096, 1, 0, 0), (16390, 2, 0, 1), (100, 4, 1, 0), (7, 8, 0, 1)],
    ]
    for spec in specs:
        members, widths, filters, methods = C3.make_set(spec, 10)
        f = M3.pack(members, widths, filters, methods)
        x = b"".join(members)
        n, entries, total = M3.check(f)
        assert M3.version_of(f) == 3 and len(f) % 16 == 0 and total == len(f) and n == len(x) and len(f) <= M3.bound([s[0] for s in spec], widths, methods)
        assert M3.unpack(f) == x and M3.unpack_size(f + bytes(16)) == (len(x), len(f))
        assert M3.frame_members_m(f) == ([s[0] for s in spec], widths, filters, methods)
        assert M3.unpack_members(f, list(range(len(members)))[::-1]) == members[::-1]
        assert M3.unpack_ranges(f, [(len(x) - 1, 1), (0, len(x))]) == [x[-1:], x]
        assert code_of(M3.unpack, f, len(x) - 1) == MM.E_SPACE
        # the earlier models do not know the frame
        assert code_of(M2.check, f) == F
        count, ext = struct.unpack("<II", f[16:24])
        assert ext == M3.ext_words([s[0] for s in spec], widths, methods) and M3.fixed_of(f) == 32 + 32 * count + 8 * ext
        for e, s in zip(entries, spec):
            assert (e[3] == e[4]) if s[3] else True
            assert sum(e[7]) == e[0] and len(e[7]) == (len(M3.segments(s[0], s[1])) if s[3] else 1)


def test_malformed_version_3_frames():
    x, f, cases = C3.malformed_cases()
    assert M3.unpack(f) == x
    for name, bad, code in cases:
        got = code_of(M3.unpack, bad)
        if code is None:
            assert code_of(M3.check, bad) == 0 and got in (F, CK), (name, got)
        else:
            assert got == code and code_of(M3.check, bad) == code, (name, got)


def test_golden_frame():
    with open(os.path.join(ROOT, "tests", "golden", C3.GOLDEN), "rb") as h:
        golden = h.read()
    members, widths, filters, methods = C3.golden_set()
    assert C3.golden_frame() == golden and len(golden) < 48 << 10
    assert M3.unpack(golden) == b"".join(members) and M3.frame_members_m(golden) == ([m[0] for m in C3.GOLDEN_MEMBERS], widths, filters, methods)
    count, ext = struct.unpack("<II", golden[16:24])
    assert (count, ext) == (4, 2)


def test_library_host_arithmetic_against_the_model(pkg):
    assert set(pkg.MEMBERS_EXPORTS) >= {"bwts_pack_members_bound_m", "bwts_pack_members_m_device", "bwts_pack_members_m", "bwts_frame_members_m"}
    members, widths, filters, methods = C3.golden_set()
    f = C3.golden_frame()
    lengths = [len(m) for m in members]
    assert pkg.frame_members(f) == (lengths, widths) and pkg.frame_member_filters(f) == filters and pkg.frame_member_methods(f) == methods
    assert pkg.frame_member_methods(C2.member_frame()) == [0] * len(C2.LENGTHS) and pkg.frame_member_methods(C.member_frame()) == [0] * len(C.LENGTHS)
    assert pkg.unpack_size(f) == (sum(lengths), len(f)) and pkg.unpack_size(f + bytes(32)) == (sum(lengths), len(f))
    assert pkg.pack_members_bound(lengths, widths, methods) == M3.bound(lengths, widths, methods)
    assert pkg.pack_members_bound(lengths, widths, [0] * 4) == pkg.pack_members_bound(lengths) == MM.bound(lengths)
    ls, ws, ms = [16385, 100, 32768, 9], [2, 4, 4, 8], [1, 1, 1, 0]
    assert pkg.pack_members_bound(ls, ws, ms) == M3.bound(ls, ws, ms)
    plan = pkg.debug_unpack_ranges_plan(f, [(lengths[0] - 5, 10)])
    assert plan["blocks"] == 2 and plan["covered_bytes"] == lengths[0] + lengths[1]
    x, g, cases = C3.malformed_cases()
    for name, bad, code in cases:
        first = 0 if code is None else code
        for fn in (pkg.frame_members, pkg.frame_member_methods, pkg.unpack_size):
            try:
                fn(bad)
                got = 0
            except pkg.BwtsError as e:
                got = e.code
            assert got == first, (name, fn.__name__, got, first)


def test_plan_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "members_v3_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "members_v3_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.decode().strip().endswith("checks ok")


def test_size_pin():
    """The direct method pays on weights and costs on a walk.  256 KiB each, member frames of one member: bf16 gaussian weights pack to
    213984 bytes through the chain at width 2 and to 179408 coded directly (stream bytes 179328 against 213920; the direct frame adds
    32 + 32 + 16 of header, entry and table), 0.838 of it (the bar: below 0.85); the int32 walk packs to 71632 bytes through the chain
    at width 4 and to 128000 coded directly (stream bytes 127904 against 71568, and 32 table bytes)."""
    walk, bf16 = M2.walk_i32(), M2.bf16_gaussian()
    chain, direct = len(M3.pack([bf16], [2], None, [0])), len(M3.pack([bf16], [2], None, [1]))
    print("bf16 gaussian: %d -> %d bytes, %.4f" % (chain, direct, direct / chain))
    assert (chain, direct) == (213920 + 64, 179328 + 64 + 16) and direct < 0.85 * chain
    chain, direct = len(M3.pack([walk], [4], None, [0])), len(M3.pack([walk], [4], None, [1]))
    print("i32 walk: %d -> %d bytes, %.4f" % (chain, direct, direct / chain))
    assert (chain, direct) == (71568 + 64, 127904 + 64 + 32) and direct > chain
