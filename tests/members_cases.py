"""What the member frame's suites share (include/bwts_members.h): the member set that meets every boundary, its model frame (made
once), the malformed frames, one per refusal of the header's list, and the range sets across member boundaries."""
import functools
import struct

import pack_members_model as MM
import pack_v3_model as P3
from test_pack_model import _put, _reseal_header_only, fixture_input

# shorter than a width and tails: 1, 2, 7, 8, 9; 8193 at width 2: q = 4096 and a tail of 1, a tile without elements; 32775 at width 8:
# one full tile and a tail; block edges 4095, 4096, 4097; 16385 crosses a coder tile, 65537 lies just past 64 KiB, 262145 crosses the
# 256 KiB table block.  The widths cycle 1, 2, 4, 8, so every width meets a start at no alignment.
LENGTHS = [1, 2, 7, 8, 9, 8193, 4095, 32775, 4096, 4097, 16385, 65537, 262145]
WIDTHS = [(1, 2, 4, 8)[k % 4] for k in range(len(LENGTHS))]
assert sum(LENGTHS) < 1 << 20 and dict(zip(LENGTHS, WIDTHS))[8193] == 2 and dict(zip(LENGTHS, WIDTHS))[32775] == 8


@functools.lru_cache(maxsize=None)
def member_set():
    """(members, widths): the contents cycle text, the float32 field of the size tables, zeros."""
    members = []
    for k, ln in enumerate(LENGTHS):
        kind = k % 3
        members.append(fixture_input(ln, 100 + k) if kind == 0 else P3.f32_field(-(-ln // 4), seed=k)[:ln] if kind == 1 else bytes(ln))
    return members, list(WIDTHS)


@functools.lru_cache(maxsize=None)
def member_frame():
    members, widths = member_set()
    return MM.pack(members, widths)


# -- malformed frames ---------------------------------------------------------------------------------------------------
SMALL_LENGTHS = [4096, 4096, 100, 9]
SMALL_WIDTHS = [4, 1, 2, 8]


@functools.lru_cache(maxsize=None)
def small_set():
    return [fixture_input(4096, 5), fixture_input(4096, 6), fixture_input(100, 7), fixture_input(9, 8)], list(SMALL_WIDTHS)


# name: (members, widths) of the committed frames under tests/golden/ (tests/golden/make_golden_pack_members.py writes them)
def fixtures():
    return {"members_four_mixed.bin": small_set(), "members_one_w4.bin": ([P3.f32_field(750, seed=9) + b"\x01"], [4])}


# the malformed frames whose header and directory are sound: a stage or a checksum refuses them, and only where their member is read
BEHIND_THE_CHECKS = ("a stream that names another length", "stream magic changed")


def frame_code(name, code):
    """What the frame checks alone make of a malformed case that unpack refuses with `code`."""
    return 0 if code == MM.E_CHECKSUM or name in BEHIND_THE_CHECKS else code


def malformed_cases():
    """(x, f, cases): the concatenation, its valid frame of four members, and (name, frame, code) in the order of the header's list,
    one malformed frame per line; where a later check is meant, the CRCs are made right again."""
    members, widths = small_set()
    x = b"".join(members)
    f = MM.pack(members, widths)
    n, entries, _ = MM.check(f)
    count = len(entries)
    fixed = 32 + 32 * count
    at = MM._stream_at(entries)
    streams = [f[at[k]:at[k + 1]] for k in range(count)]
    assert entries[0][3] <= 4095          # (member 0 is coded shorter than it is: "the first len one short" needs it)

    def frame(ents, strs=streams, n=n, count=count):
        return MM.assemble(n, count, ents, strs)

    def entry(k, **kw):
        e = dict(zip(("sb", "crc", "w", "coded", "len"), entries[k]))
        e.update(kw)
        return (e["sb"], e["crc"], e["w"], e["coded"], e["len"])

    def with_entry(k, **kw):
        return frame([entry(j, **kw) if j == k else entry(j) for j in range(count)])

    F, R, C = MM.E_FORMAT, MM.E_RANGE, MM.E_CHECKSUM
    v3 = P3.pack(x[:8192], 4, 4096)
    cases = [
        # 1. the length
        ("cut to 32 bytes", f[:32], F),
        ("cut to 48 bytes", f[:48], F),
        ("8 bytes too many", f + bytes(8), F),
        # 2. magic and version
        ("wrong magic", MM.reseal(_put(f, 0, "<I", 0x4D545743)), F),
        ("version 2", MM.reseal(_put(f, 4, "<I", 2)), F),
        ("version 0", MM.reseal(_put(f, 4, "<I", 0)), F),
        ("a version-3 body of the other magic under this one", MM.reseal(_put(v3, 0, "<I", MM.MAGIC)), F),
        ("the same with the version word made 1", MM.reseal(_put(_put(v3, 0, "<I", MM.MAGIC), 4, "<I", 1)), F),
        # 3. the header CRC
        ("header CRC wrong", _put(f, 28, "<I", struct.unpack("<I", f[28:32])[0] ^ 1), F),
        # 4. n
        ("n = 0", MM.reseal(_put(f, 8, "<Q", 0)), F),
        ("n = 2^32 + 1", MM.reseal(_put(f, 8, "<Q", (1 << 32) + 1)), R),
        # 5. count
        ("count = 0", MM.reseal(_put(f, 16, "<Q", 0)), F),
        ("count = n + 1", MM.reseal(_put(f, 16, "<Q", n + 1)), F),
        ("count = 2^20 + 1 in a frame of 2^21 bytes", MM.reseal(_put(_put(f, 16, "<Q", (1 << 20) + 1), 8, "<Q", 1 << 21)), R),
        # 6. the directory inside the frame
        ("count = 2^20: a directory longer than the frame", MM.reseal(_put(_put(f, 16, "<Q", 1 << 20), 8, "<Q", 1 << 21)), F),
        ("cut inside the directory", MM.reseal(f[:32 + 64]), F),
        # 7. the directory CRC
        ("directory CRC wrong", _reseal_header_only(_put(f, 24, "<I", struct.unpack("<I", f[24:28])[0] ^ 0x100)), F),
        ("directory byte changed, CRC left", _put(f, 32 + 32 + 8, "<B", f[32 + 32 + 8] ^ 1), F),
        # 8. the entries: width, len, coded_bytes, stream_bytes
        ("width word 0", with_entry(1, w=0), F),
        ("width word 3", with_entry(0, w=3), F),
        ("width word 16", with_entry(3, w=16), F),
        ("width word 4 with its upper half set", with_entry(0, w=0x10004), F),
        ("len = 0", with_entry(2, len=0), F),
        ("a running sum of the lengths above n", with_entry(1, len=n), F),
        ("len = 2^64 - 1", with_entry(0, len=(1 << 64) - 1), F),
        ("coded_bytes = 0", with_entry(1, coded=0), F),
        ("coded_bytes = len + 1", with_entry(2, coded=101), F),
        ("stream_bytes no multiple of 16", with_entry(1, sb=entries[1][0] + 8), F),
        ("stream_bytes = 0", with_entry(1, sb=0), F),
        ("stream_bytes beyond the coder's bound", with_entry(3, sb=1 << 20), F),
        # 9. the sum of the lengths
        ("the lengths add up to less than n", frame([entry(j) for j in range(count)], n=n + 1), F),
        ("the first len one short", with_entry(0, len=4095), F),
        # 10. the frame's length
        ("cut by 16", MM.reseal(f[:-16]), F),
        ("16 bytes too many", f + bytes(16), F),
        ("one stream 16 bytes longer in the directory", with_entry(0, sb=entries[0][0] + 16), F),
        # behind the checks: the stages' own refusals and the checksums
        ("a stream that names another length", frame([entry(0, coded=entries[0][3] - 1), entry(1), entry(2), entry(3)]), F),
        ("stream magic changed", _put(f, at[1], "<I", 0), F),
        ("two members of one length swapped", frame([entry(1, crc=entries[0][1]), entry(0, crc=entries[1][1]), entry(2), entry(3)],
                                                  [streams[1], streams[0], streams[2], streams[3]]), C),
        ("a checksum changed", with_entry(2, crc=entries[2][1] ^ 1), C),
        # in bounds, but joined at another width than the member was split at
        ("width 4 rewritten to 2", with_entry(0, w=2), C),
        ("width 4 rewritten to 8", with_entry(0, w=8), C),
        ("width 4 rewritten to 1", with_entry(0, w=1), C),
        ("width 1 rewritten to 4", with_entry(1, w=4), C),
    ]
    return x, f, cases


def range_sets():
    """(name, ranges) over the member set's concatenation: within one member, across two, over the whole, and around the seams."""
    off = [0]
    for ln in LENGTHS:
        off.append(off[-1] + ln)
    n = off[-1]
    k4096, k65537 = LENGTHS.index(4096), LENGTHS.index(65537)
    return [
        ("first byte", [(0, 1)]),
        ("last byte", [(n - 1, 1)]),
        ("within one member", [(off[k65537] + 1000, 5000)]),
        ("one member exactly", [(off[k4096], 4096)]),
        ("across two members", [(off[k4096] - 3, 10)]),
        ("straddles a seam by a byte each side", [(off[k65537] - 1, 2)]),
        ("the short members at the front, each by a byte", [(off[k], 1) for k in range(5)]),
        ("an uncovered member between two ranges", [(off[5] + 7, 100), (off[7] + 7, 100)]),
        ("descending, overlapping, a repeat", [(off[10] + 5, 40), (off[6], 4095 + 32775), (off[10] + 5, 40), (3, 20)]),
        ("whole input", [(0, n)]),
    ]
