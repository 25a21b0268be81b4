"""CPU suite of the packed frame, version 2 (include/bwts_pack.h): the model (tests/pack_v2_model.py) against itself and against the
version-1 model, the committed version-2 fixtures, the list of malformed version-2 frames that the GPU suite shares, the library's
host arithmetic against the model, and the sizes the zero-run stage is there for."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

import ec_model as E
import oracle_lib as O
import pack_model as P1
import pack_v2_model as P
import realtext
import zrl_model as Z
from test_pack_model import B0, ROUND_TRIP_B, ROUND_TRIP_N, _put, _reseal_header_only, fixture_input, malformed_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"pack_v2_one_block.bwz": (fixture_input(3001, 1), 0), "pack_v2_three_blocks.bwz": (fixture_input(2 * B0 + 777, 2), B0)}


@pytest.mark.parametrize("n", ROUND_TRIP_N)
def test_model_round_trip(n):
    x = fixture_input(n, n)
    for B in ROUND_TRIP_B:
        f = P.pack(x, B)
        real_b = n if B == 0 or B >= n else B
        ls = P.lengths(n, real_b)
        assert len(f) % 16 == 0 and len(f) <= P.bound(n, B)
        assert struct.unpack("<IIQQ", f[:24]) == (P.MAGIC, 2, n, real_b)
        assert P.unpack_size(f) == (n, len(f)) and P.unpack_size(f + bytes(32)) == (n, len(f))
        assert P.unpack(f) == x
        # the streams are what the coder's segment form writes for the coded_bytes lengths, over the zero-run stage's segment output
        version, _, _, entries, _ = P.check(f)
        ranks = b"".join(P.ranks(x[at:at + real_b]).tobytes() for at in range(0, n, real_b))
        coded = Z.encode_segments(ranks, ls)
        assert version == 2 and [e[2] for e in entries] == [len(c) for c in coded]
        assert f[32 + 32 * len(ls):] == b"".join(E.encode_segments(b"".join(coded), [len(c) for c in coded]))
        # a version-1 frame of the same input goes through the same check and unpack
        g = P1.pack(x, B)
        assert P.check(g)[0] == 1 and P.unpack(g) == x and P.unpack_size(g) == (n, len(g))


def test_model_arguments():
    assert P.bound(5000, 100) == 0 and P.bound(1, 0) == 64 + E.bound(1) and P.bound(1, 0, version=1) == P1.bound(1, 0) and P.bound(1, 0, version=3) == 0
    assert P.bound(3 * B0 + 1, B0) == P1.bound(3 * B0 + 1, B0) + 16 * 4
    with pytest.raises(P.PackError) as e:
        P.pack(bytes(5000), 100)
    assert e.value.code == P.E_ARG
    with pytest.raises(P.PackError) as e:
        P.unpack(P.pack(b"abc"), out_cap=2)
    assert e.value.code == P.E_SPACE


def test_committed_fixtures_are_the_models_output():
    for name, (x, B) in FIXTURES.items():
        got = open(os.path.join(GOLDEN, name), "rb").read()
        assert 512 < len(got) < 16384, name
        assert got == P.pack(x, B), name
        assert P.unpack(got) == x, name
    assert struct.unpack("<IQQ", open(os.path.join(GOLDEN, "pack_v2_three_blocks.bwz"), "rb").read()[4:24]) == (2, 2 * B0 + 777, B0)


# -- malformed frames ---------------------------------------------------------------------------------------
def malformed_cases():
    """(name, frame, code): version-1's conditions carried over to the 32-byte entries, then what version 2 adds; shared with the GPU
    suite, which must see each refused by the model with that code first."""
    x = malformed_input()
    f = P.pack(x, B0)
    _, n, B, entries, _ = P.check(f)
    sb, crcs, cb = [e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries]
    fixed = 32 + 32 * 3
    at = [fixed, fixed + sb[0], fixed + sb[0] + sb[1], len(f)]
    streams = [f[at[k]:at[k + 1]] for k in range(3)]
    coded = [Z.encode(P.ranks(x[k * B0:(k + 1) * B0])) for k in range(3)]
    assert [len(c) for c in coded] == cb and all(c < ln for c, ln in zip(cb, P.lengths(n, B)))
    one = P.pack(x[:B0])

    def frame(ents, strs):
        return P.assemble(n, B, ents, strs)

    def entry(k, **kw):
        e = {"sb": sb[k], "crc": crcs[k], "rsv": 0, "coded": cb[k], "rsv2": 0}
        e.update(kw)
        return (e["sb"], e["crc"], e["rsv"], e["coded"], e["rsv2"])

    def with_stream(k, z, **kw):
        """block k's stream replaced by the coder's stream of z"""
        s = E.encode(z)
        return frame([entry(j, sb=len(s), **kw) if j == k else entry(j) for j in range(3)], [s if j == k else streams[j] for j in range(3)])

    bad_zrl = coded[1][:-1] + b"\xff"                               # a 255 as the last byte: the coder's stream of it is sound
    assert Z.decode(bad_zrl, B0) is None
    F, R, C = P.E_FORMAT, P.E_RANGE, P.E_CHECKSUM
    cases = [
        ("cut to 32 bytes", f[:32], F),
        ("cut to 48 bytes", f[:48], F),
        ("cut inside the directory", f[:32 + 64], F),
        ("8 bytes too many", f + bytes(8), F),
        ("wrong magic", P.reseal(_put(f, 0, "<I", 0x5A545743)), F),
        ("version 3", P.reseal(_put(f, 4, "<I", 3)), F),
        ("version 1 over a version-2 body", P.reseal(_put(f, 4, "<I", 1)), F),
        ("header CRC wrong", _put(f, 28, "<I", struct.unpack("<I", f[28:32])[0] ^ 1), F),
        ("n = 0", P.reseal(_put(f, 8, "<Q", 0)), F),
        ("n = 2^32 + 1", P.reseal(_put(f, 8, "<Q", (1 << 32) + 1)), R),
        ("B = 0", P.reseal(_put(f, 16, "<Q", 0)), F),
        ("B > n", P.reseal(_put(f, 16, "<Q", n + 1)), F),
        ("B = 4095 < n", P.reseal(_put(f, 16, "<Q", 4095)), F),
        ("directory longer than the frame", P.reseal(_put(f, 8, "<Q", 1 << 32)), F),
        ("directory CRC wrong", _reseal_header_only(_put(f, 24, "<I", struct.unpack("<I", f[24:28])[0] ^ 0x100)), F),
        ("directory byte changed, CRC left", _put(f, 32 + 32 + 8, "<B", f[32 + 32 + 8] ^ 1), F),
        ("nonzero reserved word", frame([entry(0), entry(1, rsv=1), entry(2)], streams), F),
        ("second reserved word nonzero", frame([entry(0), entry(1, rsv2=1), entry(2)], streams), F),
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
        ("one block: stream names coded_bytes + 1", P.assemble(B0, B0, [(sb[0], crcs[0], 0, cb[0] - 1, 0)], [streams[0]]), F),
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
    assert codes.count(P.E_CHECKSUM) >= 3 and codes.count(P.E_RANGE) == 1
    for name, bad, code in cases:
        with pytest.raises(P.PackError) as e:
            P.unpack(bad)
        assert e.value.code == code, name


# -- the library's host arithmetic (no device) ------------------------------------------------------
def test_library_bound_against_the_model(pkg):
    L = pkg.lib()
    for n in ROUND_TRIP_N + [1 << 20, (1 << 32) - 1, 1 << 32]:
        for B in ROUND_TRIP_B + [65536, 1 << 33]:
            assert L.bwts_pack_bound_v(2, n, B) == P.bound(n, B), (n, B)
            assert L.bwts_pack_bound_v(1, n, B) == P1.bound(n, B) == L.bwts_pack_bound(n, B), (n, B)
            if P.bound(n, B):
                assert pkg.pack_bound(n, B, version=2) == P.bound(n, B) and pkg.pack_bound(n, B) == P1.bound(n, B)
    for v in (1, 2):
        assert L.bwts_pack_bound_v(v, 0, 0) == 0 and L.bwts_pack_bound_v(v, (1 << 32) + 1, 0) == 0 and L.bwts_pack_bound_v(v, 5000, 4095) == 0
    assert L.bwts_pack_bound_v(0, 100, 0) == 0 and L.bwts_pack_bound_v(3, 100, 0) == 0
    with pytest.raises(pkg.BwtsError):
        pkg.pack_bound(100, 0, version=3)


def test_library_unpack_size_against_the_model(pkg):
    x, f, cases = malformed_cases()
    assert pkg.unpack_size(f) == (len(x), len(f))
    g = P1.pack(x, B0)
    assert pkg.unpack_size(f + g[:48]) == (len(x), len(f)) and pkg.unpack_size(g + f[:64]) == (len(x), len(g))      # concatenated frames of both versions
    for name, (y, B) in FIXTURES.items():
        h = P.pack(y, B)
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


# -- what the stage is there for ---------------------------------------------------------------------------
def _u8(x):
    return x if isinstance(x, bytes) else np.ascontiguousarray(x, dtype=np.uint8).tobytes()


def test_frames_of_compressible_inputs_are_smaller():
    for name, x in (("text", _u8(O.generate("text", 1 << 18, 3))), ("realtext", _u8(realtext.corpus(1 << 20))), ("repeat", b"\x71" * 70001)):
        v1, v2 = P1.pack(x), P.pack(x)
        assert len(v2) < len(v1), (name, len(v1), len(v2))


def test_frames_of_other_inputs_grow_by_the_directory_alone():
    for name, n in (("zipf", 1 << 18), ("uniform256", 1 << 16)):
        x = _u8(O.generate(name, n, 3))
        for B in (0, 1 << 16):
            nblk = len(P.lengths(n, P.block_len(n, B)))
            v1, v2 = P1.pack(x, B), P.pack(x, B)
            assert len(v2) <= len(v1) + 16 * nblk, (name, B, len(v1), len(v2))
