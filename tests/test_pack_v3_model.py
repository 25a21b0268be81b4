"""CPU suite of the packed frame, version 3 (include/bwts_pack.h): the model (tests/pack_v3_model.py) against itself and against the
models of versions 1 and 2, the committed version-3 fixtures, the list of malformed version-3 frames that the GPU suite shares, the
library's host arithmetic against the model, and the sizes the byte-plane split is there for."""
import os
import struct

import numpy as np
import pytest

import ec_model as E
import pack_model as P1
import pack_v2_model as P2
import pack_v3_model as P
import planes_model as S
import zrl_model as Z
from test_pack_model import B0, ROUND_TRIP_B, ROUND_TRIP_N, _put, _reseal_header_only, fixture_input, malformed_input
from test_pack_v2_model import malformed_cases as v2_malformed_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def typed_input(n, seed):
    """n bytes that look like an array of little-endian int32 values on a slow walk: integer arithmetic alone, like fixture_input."""
    out, x, v = bytearray(), seed, 1 << 20
    while len(out) < n:
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        v = (v + (x >> 33) % 101 - 50) & 0xFFFFFFFF
        out += struct.pack("<I", v)
    return bytes(out[:n])


# name: (input, width, block_bytes); the blocks of the second are no multiple of its width
FIXTURES = {"pack_v3_one_block_w4.bin": (typed_input(3001, 1), 4, 0), "pack_v3_three_blocks_w8.bin": (typed_input(2 * 4097 + 777, 2), 8, 4097),
            "pack_v3_text_w2.bin": (fixture_input(2 * B0 + 1, 3), 2, B0)}


def named_lengths(w):
    """The lengths of the split's own test (tests/test_planes_model.py), per width."""
    return [1, w - 1, w, w + 1, 16 * w - 1, 4095, 4096, 4097, 70001]


@pytest.mark.parametrize("w", P.WIDTHS)
def test_model_round_trip_at_the_splits_lengths(w):
    """A frame at every length where the split has a tail or none, in one block and cut at 4096 and 4097 (blocks whose length is no
    multiple of w keep a tail each; 70001 = 17 * 4096 + 369 = 17 * 4097 + 352)."""
    for n in named_lengths(w):
        x = typed_input(n, 100 * n + w)
        for B in ROUND_TRIP_B:
            f = P.pack(x, w, B)
            real_b = n if B == 0 or B >= n else B
            ls = P.lengths(n, real_b)
            assert len(f) % 16 == 0 and len(f) <= P.bound(w, n, B)
            assert struct.unpack("<IIQQ", f[:24]) == (P.MAGIC, 3, n, real_b)
            version, _, _, entries, total, width = P.check(f)
            assert (version, width, total, len(entries)) == (3, w, len(f), len(ls))
            assert P.unpack_size(f) == (n, len(f))
            assert P.unpack(f) == x, (n, w, B)
            # the chain of every block: the split with its own tail, then version 2's
            for k, (sb, crc, coded) in enumerate(entries):
                block = x[k * real_b:(k + 1) * real_b]
                assert crc == P1.zlib.crc32(block)
                assert coded == len(Z.encode(P2.ranks(S.split(block, w).tobytes()))), (n, w, B, k)


@pytest.mark.parametrize("n", ROUND_TRIP_N)
def test_model_round_trip(n):
    x = typed_input(n, n)
    for w in P.WIDTHS:
        for B in ROUND_TRIP_B:
            f = P.pack(x, w, B)
            real_b = n if B == 0 or B >= n else B
            ls = P.lengths(n, real_b)
            assert len(f) % 16 == 0 and len(f) <= P.bound(w, n, B) == P2.bound(n, B)
            assert struct.unpack("<IIQQ", f[:24]) == (P.MAGIC, 3, n, real_b)
            assert P.unpack_size(f) == (n, len(f)) and P.unpack_size(f + bytes(32)) == (n, len(f))
            assert P.unpack(f) == x, (n, w, B)
            # every block is split on its own, and the rest is version 2's chain over the split blocks
            version, _, _, entries, _, width = P.check(f)
            assert version == 3 and width == w
            split = b"".join(S.split(x[at:at + real_b], w).tobytes() for at in range(0, n, real_b))
            g = P2.pack(split, B)
            assert f[32 + 32 * len(ls):] == g[32 + 32 * len(ls):]
            for k in range(len(ls)):
                e3 = struct.unpack("<QIIQQ", f[32 + 32 * k:64 + 32 * k])
                e2 = struct.unpack("<QIIQQ", g[32 + 32 * k:64 + 32 * k])
                assert e3[0] == e2[0] and e3[3:] == e2[3:] and e3[2] == w and e2[2] == 0
                assert e3[1] == P1.zlib.crc32(x[k * real_b:(k + 1) * real_b])          # the original bytes', not the split's


def test_a_last_block_of_one_byte():
    for w in P.WIDTHS:
        for B in (4096, 4097):
            x = typed_input(2 * B + 1, w)
            f = P.pack(x, w, B)
            assert P.lengths(len(x), B)[-1] == 1 and P.unpack(f) == x


def test_all_versions_through_the_same_check_and_unpack():
    x = typed_input(3 * B0 + 5, 9)
    for f, version, width in ((P1.pack(x, B0), 1, 0), (P2.pack(x, B0), 2, 0), (P.pack(x, 4, B0), 3, 4)):
        got = P.check(f)
        assert (got[0], got[1], got[5]) == (version, len(x), width)
        assert P.unpack(f) == x and P.unpack_size(f) == (len(x), len(f))


def test_model_arguments():
    assert P.bound(4, 5000, 100) == 0 and P.bound(4, 1, 0) == 64 + E.bound(1)
    for w in (0, 1, 3, 16):
        assert P.bound(w, 5000, 0) == 0
        with pytest.raises(P.PackError) as e:
            P.pack(bytes(5000), w)
        assert e.value.code == P.E_ARG
    with pytest.raises(P.PackError) as e:
        P.pack(bytes(5000), 4, 100)
    assert e.value.code == P.E_ARG
    with pytest.raises(P.PackError) as e:
        P.unpack(P.pack(b"abc", 2), out_cap=2)
    assert e.value.code == P.E_SPACE


def test_committed_fixtures_are_the_models_output():
    for name, (x, w, B) in FIXTURES.items():
        got = open(os.path.join(GOLDEN, name), "rb").read()
        assert 512 < len(got) < 16384, name
        assert got == P.pack(x, w, B), name
        assert P.unpack(got) == x, name
    assert struct.unpack("<IQQ", open(os.path.join(GOLDEN, "pack_v3_three_blocks_w8.bin"), "rb").read()[4:24]) == (3, 2 * 4097 + 777, 4097)


# -- malformed frames ---------------------------------------------------------------------------------------
def set_widths(frame, widths):
    g = frame
    for k, w in enumerate(widths):
        g = _put(g, 32 + 32 * k + 12, "<I", w)
    return P.reseal(g)


def malformed_cases():
    """(name, frame, code): what version 3 adds, then every version-2 refusal restated on a version-3 frame at width 4; shared with
    the GPU suite, which must see each refused by the model with that code first."""
    x = malformed_input()
    f = P.pack(x, 4, B0)
    _, n, B, entries, _, width = P.check(f)
    sb, crcs, cb = [e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries]
    fixed = 32 + 32 * 3
    at = [fixed, fixed + sb[0], fixed + sb[0] + sb[1], len(f)]
    streams = [f[at[k]:at[k + 1]] for k in range(3)]
    coded = [Z.encode(P2.ranks(S.split(x[k * B0:(k + 1) * B0], 4).tobytes())) for k in range(3)]
    assert width == 4 and [len(c) for c in coded] == cb and cb[0] < B0 and cb[1] < B0      # (the cases below need blocks 0 and 1 coded; the 100 split bytes of block 2 are stored)
    one = P.pack(x[:B0], 4)

    def frame(ents, strs):
        return P.assemble(n, B, ents, strs)

    def entry(k, **kw):
        e = {"sb": sb[k], "crc": crcs[k], "w": 4, "coded": cb[k], "rsv2": 0}
        e.update(kw)
        return (e["sb"], e["crc"], e["w"], e["coded"], e["rsv2"])

    def with_stream(k, z, **kw):
        """block k's stream replaced by the coder's stream of z"""
        s = E.encode(z)
        return frame([entry(j, sb=len(s), **kw) if j == k else entry(j) for j in range(3)], [s if j == k else streams[j] for j in range(3)])

    bad_zrl = coded[1][:-1] + b"\xff"                               # a 255 as the last byte: the coder's stream of it is sound
    assert Z.decode(bad_zrl, B0) is None
    F, R, C = P.E_FORMAT, P.E_RANGE, P.E_CHECKSUM
    cases = [("width word %d" % w, set_widths(f, [w] * 3), F) for w in (0, 1, 3, 16)]
    cases += [
        ("two entries with different widths", set_widths(f, [4, 2, 4]), F),
        ("the last entry's width differs", set_widths(f, [4, 4, 8]), F),
        ("the first entry's width is 0", set_widths(f, [0, 4, 4]), F),
        ("width word 4 with its upper half set", set_widths(f, [0x10004] * 3), F),
        ("version 2 over a version-3 body", P.reseal(_put(f, 4, "<I", 2)), F),
        ("version 3 over a version-2 body", P.reseal(_put(P2.pack(x, B0), 4, "<I", 3)), F),
        # in bounds, but joined at another width than the blocks were split at
        ("width 4 rewritten to 2", set_widths(f, [2] * 3), C),
        ("width 4 rewritten to 8", set_widths(f, [8] * 3), C),
        # version 2's list
        ("cut to 32 bytes", f[:32], F),
        ("cut to 48 bytes", f[:48], F),
        ("cut inside the directory", f[:32 + 64], F),
        ("8 bytes too many", f + bytes(8), F),
        ("wrong magic", P.reseal(_put(f, 0, "<I", 0x5A545743)), F),
        ("version 4", P.reseal(_put(f, 4, "<I", 4)), F),
        ("version 1 over a version-3 body", P.reseal(_put(f, 4, "<I", 1)), F),
        ("header CRC wrong", _put(f, 28, "<I", struct.unpack("<I", f[28:32])[0] ^ 1), F),
        ("n = 0", P.reseal(_put(f, 8, "<Q", 0)), F),
        ("n = 2^32 + 1", P.reseal(_put(f, 8, "<Q", (1 << 32) + 1)), R),
        ("B = 0", P.reseal(_put(f, 16, "<Q", 0)), F),
        ("B > n", P.reseal(_put(f, 16, "<Q", n + 1)), F),
        ("B = 4095 < n", P.reseal(_put(f, 16, "<Q", 4095)), F),
        ("directory longer than the frame", P.reseal(_put(f, 8, "<Q", 1 << 32)), F),
        ("directory CRC wrong", _reseal_header_only(_put(f, 24, "<I", struct.unpack("<I", f[24:28])[0] ^ 0x100)), F),
        ("directory byte changed, CRC left", _put(f, 32 + 32 + 8, "<B", f[32 + 32 + 8] ^ 1), F),
        ("trailing word nonzero", frame([entry(0), entry(1, rsv2=1), entry(2)], streams), F),
        ("coded_bytes = 0", frame([entry(0), entry(1, coded=0), entry(2)], streams), F),
        ("coded_bytes = block length + 1", frame([entry(0), entry(1), entry(2, coded=101)], streams), F),
        ("stream_bytes + 8", frame([entry(0), entry(1, sb=sb[1] + 8), entry(2)], streams), F),
        ("stream_bytes = 16", frame([entry(0), entry(1, sb=16), entry(2)], streams), F),
        ("stream_bytes = 2^63", frame([entry(0), entry(1), entry(2, sb=1 << 63)], streams), F),
        ("sizes add up to more", frame([entry(0, sb=sb[0] + 16), entry(1), entry(2)], streams), F),
        ("16 bytes too many", f + bytes(16), F),
        ("cut by 16", f[:-16], F),
        # what the coder refuses passes through
        ("stream magic changed", _put(f, at[1], "<I", 0x43455743), F),
        ("stream names coded_bytes + 1", with_stream(1, coded[1] + b"\x05"), F),
        ("stream names coded_bytes - 1", with_stream(1, coded[1][:-1]), F),
        ("one block: stream names coded_bytes + 1", P.assemble(B0, B0, [(sb[0], crcs[0], 4, cb[0] - 1, 0)], [streams[0]]), F),
        # ... and what the zero-run decoder refuses
        ("valid stream of an invalid zero-run input", with_stream(1, bad_zrl), F),
        ("coded_bytes = block length over coded bytes", with_stream(1, coded[1] + bytes(B0 - cb[1]), coded=B0), C),
        # in bounds, but not the bytes that were packed
        ("directory CRC of a block changed", frame([entry(0, crc=crcs[0] ^ 0x80000000), entry(1), entry(2)], streams), C),
        ("two blocks swapped", frame([entry(0, sb=sb[1], coded=cb[1]), entry(1, sb=sb[0], coded=cb[0]), entry(2)], [streams[1], streams[0], streams[2]]), C),
        ("one block: CRC changed", P.reseal(_put(one, 32 + 8, "<I", struct.unpack("<I", one[40:44])[0] ^ 1)), C),
    ]
    return x, f, cases


def test_model_refuses_malformed_frames():
    x, f, cases = malformed_cases()
    assert P.unpack(f) == x
    codes = [c for _, _, c in cases]
    assert codes.count(P.E_CHECKSUM) >= 5 and codes.count(P.E_RANGE) == 1
    # every version-2 refusal is restated: its names, but for the three whose meaning the width word changes (restated above them)
    theirs = {name for name, _, _ in v2_malformed_cases()[2]} - {"version 3", "version 1 over a version-2 body", "nonzero reserved word", "second reserved word nonzero"}
    assert theirs <= {name for name, _, _ in cases}, theirs - {name for name, _, _ in cases}
    for name, bad, code in cases:
        with pytest.raises(P.PackError) as e:
            P.unpack(bad)
        assert e.value.code == code, name


def test_version_2_frames_are_judged_as_before():
    """Version 2's own list through the version-3 model: the same codes."""
    x, f, cases = v2_malformed_cases()
    assert P.unpack(f) == x
    for name, bad, code in cases:
        with pytest.raises(P.PackError) as e:
            P.unpack(bad)
        assert e.value.code == code, name


# -- the library's host arithmetic (no device) ------------------------------------------------------
def test_library_bound_against_the_model(pkg):
    L = pkg.lib()
    for n in ROUND_TRIP_N + [1 << 20, (1 << 32) - 1, 1 << 32]:
        for B in ROUND_TRIP_B + [65536, 1 << 33]:
            for w in P.WIDTHS:
                assert L.bwts_pack_planes_bound(w, n, B) == P.bound(w, n, B), (w, n, B)
                if P.bound(w, n, B):
                    assert pkg.pack_bound(n, B, planes=w) == P.bound(w, n, B) == pkg.pack_bound(n, B, version=3, planes=w)
            for w in (0, 1, 3, 16):
                assert L.bwts_pack_planes_bound(w, n, B) == 0
    for w in P.WIDTHS:
        assert L.bwts_pack_planes_bound(w, 0, 0) == 0 and L.bwts_pack_planes_bound(w, (1 << 32) + 1, 0) == 0 and L.bwts_pack_planes_bound(w, 5000, 4095) == 0
    # version 3 is asked for with a width, never through the version alone; planes goes with no other version
    assert L.bwts_pack_bound_v(3, 100, 0) == 0
    for kw in ({"version": 3}, {"version": 1, "planes": 4}, {"version": 2, "planes": 4}, {"planes": 3}):
        with pytest.raises(pkg.BwtsError):
            pkg.pack_bound(100, 0, **kw)


def test_library_unpack_size_against_the_model(pkg):
    x, f, cases = malformed_cases()
    assert pkg.unpack_size(f) == (len(x), len(f))
    g1, g2 = P1.pack(x, B0), P2.pack(x, B0)
    assert pkg.unpack_size(f + g1[:48]) == (len(x), len(f)) and pkg.unpack_size(g2 + f[:64]) == (len(x), len(g2))      # concatenated frames of all versions
    for name, (y, w, B) in FIXTURES.items():
        h = P.pack(y, w, B)
        assert pkg.unpack_size(h) == (len(y), len(h))
    for name, bad, code in cases:
        try:
            want = P.unpack_size(bad)
        except P.PackError as e:
            with pytest.raises(pkg.BwtsError) as got:
                pkg.unpack_size(bad)
            assert got.value.code == e.code, name
        else:
            assert pkg.unpack_size(bad) == want, name                 # what only the streams, the zero-run inputs or the checksums show


# -- what the stage is there for, and where it gains nothing ---------------------------------------------------
def test_a_smooth_f32_field_packs_a_fifth_smaller_at_least():
    """65 536 float32 values, 256 KiB: measured 168 800 bytes at width 4 against 254 112 for version 2, a ratio of 0.664."""
    x = P.f32_field(65536)
    v2, v3 = P2.pack(x), P.pack(x, 4)
    print("f32 field: version 2 %d bytes, version 3 at width 4 %d bytes, ratio %.4f" % (len(v2), len(v3), len(v3) / len(v2)))
    assert P.unpack(v3) == x
    assert len(v3) < 0.8 * len(v2)


def test_bf16_noise_gains_nothing_and_loses_nothing():
    """65 536 bf16 gaussian weights: the split neither helps nor hurts by more than 2 % (measured +0.4 %): the honest no-gain case."""
    x = P.bf16_gaussian(65536)
    v2, v3 = P2.pack(x), P.pack(x, 2)
    print("bf16 gaussian: version 2 %d bytes, version 3 at width 2 %d bytes, ratio %.4f" % (len(v2), len(v3), len(v3) / len(v2)))
    assert P.unpack(v3) == x
    assert abs(len(v3) - len(v2)) <= 0.02 * len(v2)
