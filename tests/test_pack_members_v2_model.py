"""CPU suite of version 2 of the member frame (include/bwts_members.h): the model (tests/pack_members_v2_model.py) round trips, a pack
without a filter is the version-1 frame, the malformed version-2 frames are refused with their codes, the library's host arithmetic
(bwts_frame_members, bwts_frame_members_f, bwts_unpack_size) agrees with the model, and the size pin of the delta filter."""
import struct

import members_cases as C
import members_v2_cases as C2
import pack_members_model as MM
import pack_members_v2_model as M2


def code_of(fn, *args):
    try:
        fn(*args)
        return 0
    except MM.PackError as e:
        return e.code


def test_a_pack_without_a_filter_is_the_version_1_frame():
    members, widths = C.small_set()
    want = MM.pack(members, widths)
    assert M2.pack(members, widths) == want and M2.pack(members, widths, [0] * 4) == want and M2.pack(members, None, None) == MM.pack(members, None)
    assert M2.version_of(want) == 1 and M2.unpack(want) == b"".join(members)
    assert M2.frame_members_f(want) == (C.SMALL_LENGTHS, C.SMALL_WIDTHS, [0] * 4)
    for ls, ws, fs, code in (([4], [4], [2], MM.E_ARG), ([4], [4], [1, 0], MM.E_ARG), ([], None, None, MM.E_ARG), ([4, 0], None, [1, 1], MM.E_ARG),
                             ([1 << 32, 1], None, [1, 1], MM.E_RANGE)):
        assert code_of(M2.check_args, ls, ws, fs) == code, (ls, ws, fs)


def test_version_2_frame_and_its_readers():
    members, widths, filters = C2.member_set()
    f = C2.member_frame()
    x = b"".join(members)
    assert M2.version_of(f) == 2 and len(f) % 16 == 0 and len(f) <= MM.bound(C2.LENGTHS)
    n, entries, total = M2.check(f)
    assert n == len(x) and total == len(f) and M2.unpack_size(f + bytes(32)) == (len(x), len(f))
    assert M2.frame_members_f(f) == (C2.LENGTHS, widths, filters)
    # the word: width below, filter above, and the checksum is the original bytes'
    for k, (ln, w, fl) in enumerate(C2.MEMBERS):
        _, crc, wf, _, elen = struct.unpack("<QIIQQ", f[32 + 32 * k:64 + 32 * k])
        assert (wf, elen) == (w | fl << 8, ln) and crc == MM.zlib.crc32(members[k])
    # the version-1 model does not know the frame
    assert code_of(MM.check, f) == MM.E_FORMAT
    assert M2.unpack(f) == x
    assert M2.unpack_members(f, [7, 0, 7, 4]) == [members[7], members[0], members[7], members[4]]
    for name, rs in C2.range_sets():
        assert M2.unpack_ranges(f, rs) == [x[o:o + nb] for o, nb in rs], name
    assert code_of(M2.unpack, f, len(x) - 1) == MM.E_SPACE
    assert code_of(M2.unpack_members, f, [len(members)]) == MM.E_RANGE and code_of(M2.unpack_members, f, []) == MM.E_ARG
    # the streams of the unfiltered members are those of the version-1 frame of the same members
    plain = MM.pack(members, widths)
    _, pe, _ = MM.check(plain)
    for k, fl in enumerate(filters):
        if not fl:
            assert entries[k][:5] == pe[k]
    # one member, filtered
    one = M2.pack([members[5]], [8], [1])
    assert M2.unpack(one) == members[5] and M2.frame_members_f(one) == ([32775], [8], [1])


def test_malformed_version_2_frames():
    x, f, cases = C2.malformed_cases()
    assert M2.unpack(f) == x
    for name, bad, code in cases:
        assert code_of(M2.unpack, bad) == code, name
        first = 0 if code == MM.E_CHECKSUM else code
        assert code_of(M2.check, bad) == first, name
        if code == MM.E_CHECKSUM:
            # a member the rewritten word does not touch is read as before
            assert M2.unpack_members(bad, [3]) == [x[-9:]]
            assert code_of(M2.unpack_ranges, bad, [(0, len(x))]) == code, name


def test_library_host_arithmetic_against_the_model(pkg):
    assert set(pkg.MEMBERS_EXPORTS) >= {"bwts_pack_members_f_device", "bwts_pack_members_f", "bwts_frame_members_f"}
    members, widths, filters = C2.member_set()
    f = C2.member_frame()
    assert pkg.frame_members(f) == (C2.LENGTHS, widths) and pkg.frame_member_filters(f) == filters
    assert pkg.unpack_size(f) == (sum(C2.LENGTHS), len(f)) and pkg.unpack_size(f + bytes(32)) == (sum(C2.LENGTHS), len(f))
    assert pkg.frame_member_filters(C.member_frame()) == [0] * len(C.LENGTHS)
    plan = pkg.debug_unpack_ranges_plan(f, [(sum(C2.LENGTHS[:4]) - 5, 10)])
    assert plan["blocks"] == 2 and plan["covered_bytes"] == C2.LENGTHS[3] + C2.LENGTHS[4]
    x, g, cases = C2.malformed_cases()
    assert pkg.frame_members(g) == (C.SMALL_LENGTHS, C.SMALL_WIDTHS) and pkg.frame_member_filters(g) == C2.SMALL_FILTERS
    for name, bad, code in cases:
        first = 0 if code == MM.E_CHECKSUM else code
        for fn in (pkg.frame_members, pkg.frame_member_filters, pkg.unpack_size):
            try:
                fn(bad)
                got = 0
            except pkg.BwtsError as e:
                got = e.code
            assert got == first, (name, fn.__name__, got, first)


def test_size_pin():
    """The delta filter pays on an integer random walk and costs little where it does not.  256 KiB each, member frames of one member:
    the int32 walk (steps uniform in [-50, 50]) packs to 71632 bytes at width 4 and to 56240 with the filter, 0.785 of it (the bar:
    below 0.85); bf16 gaussian weights pack to 213984 bytes at width 2 and to 220720 with the filter, 3.1 % more (the bar: within 5 %)."""
    walk, bf16 = M2.walk_i32(), M2.bf16_gaussian()
    assert len(walk) == len(bf16) == 1 << 18
    plain, filtered = len(M2.pack([walk], [4], [0])), len(M2.pack([walk], [4], [1]))
    print("i32 walk: %d -> %d bytes, %.4f" % (plain, filtered, filtered / plain))
    assert (plain, filtered) == (71632, 56240) and filtered < 0.85 * plain
    plain, filtered = len(M2.pack([bf16], [2], [0])), len(M2.pack([bf16], [2], [1]))
    print("bf16 gaussian: %d -> %d bytes, %.4f" % (plain, filtered, filtered / plain))
    assert (plain, filtered) == (213984, 220720) and filtered <= 1.05 * plain
