"""What the suites of version 3 of the member frame share (include/bwts_members.h): the golden member set, weight-like and text-like
members of any length, and the malformed version-3 frames with the model's codes."""
import functools
import struct

import numpy as np

import pack_members_model as MM
import pack_members_v3_model as M3
from test_pack_model import fixture_input

GOLDEN = "members_v3_mixed.bin"
# (length, width, filter, method): a chain member of width 1; a direct member of width 2 with separate planes and a 1-byte tail; a
# direct member of width 4 below the plane minimum; a direct member of width 8 with the delta filter
GOLDEN_MEMBERS = [(3000, 1, 0, 0), (2 * 8192 + 1, 2, 0, 1), (4 * 1000 + 3, 4, 0, 1), (8 * 300, 8, 1, 1)]


def weights(ln, w, seed):
    """ln bytes of gaussian weights (sigma 0.02): bfloat16 at width 2, float32 at width 4, float64 at width 8, their low bytes at width 1."""
    q = -(-ln // w)
    x = np.random.default_rng(seed).standard_normal(q) * 0.02
    if w == 2:
        b = (x.astype("<f4").view("<u4") >> 16).astype("<u2").tobytes()
    elif w == 4:
        b = x.astype("<f4").tobytes()
    elif w == 8:
        b = x.astype("<f8").tobytes()
    else:
        b = (x.astype("<f4").view("<u4") & 0xFF).astype("u1").tobytes()
    return b[:ln]


def walk(ln, w, seed):
    """ln bytes of a random walk of w-byte little-endian integers: what the delta filter is for."""
    q = -(-ln // w)
    steps = np.random.default_rng(seed).integers(-300, 301, q).astype(np.int64)
    a = (np.cumsum(steps) + (1 << (8 * w - 2))).astype(np.uint64)
    return a.astype({1: "u1", 2: "<u2", 4: "<u4", 8: "<u8"}[w]).tobytes()[:ln]


def member(ln, w, f, m, seed):
    """A member for its method: weights where it is direct, a walk where it is filtered, else text."""
    if f:
        return walk(ln, w, seed)
    return weights(ln, w, seed) if m else fixture_input(ln, 300 + seed)


def make_set(spec, seed=0):
    """(members, widths, filters, methods) of a list of (length, width, filter, method)."""
    return ([member(ln, w, f, m, seed + k) for k, (ln, w, f, m) in enumerate(spec)], [s[1] for s in spec], [s[2] for s in spec],
            [s[3] for s in spec])


@functools.lru_cache(maxsize=None)
def golden_set():
    return make_set(GOLDEN_MEMBERS, 70)


@functools.lru_cache(maxsize=None)
def golden_frame():
    return M3.pack(*golden_set())


def parts(f):
    """A valid version-3 frame taken apart: (n, entries as assemble takes them, table words, streams one per member)."""
    n, entries, _ = M3.check(f)
    count, ext = struct.unpack("<II", f[16:24])
    table = list(struct.unpack("<%dQ" % ext, f[32 + 32 * count:32 + 32 * count + 8 * ext]))
    at = [M3.fixed_of(f)]
    for e in entries:
        at.append(at[-1] + e[0])
    ents = [(e[0], e[1], M3.word(e[2], e[5], e[6]), e[3], e[4]) for e in entries]
    return n, ents, table, [f[at[k]:at[k + 1]] for k in range(len(entries))]


def _entry(ents, k, **kw):
    names = ("stream_bytes", "crc", "word", "coded", "len")
    e = list(ents[k])
    for name, v in kw.items():
        e[names.index(name)] = v
    return [tuple(e) if j == k else ents[j] for j in range(len(ents))]


def malformed_cases():
    """(x, f, cases): the golden concatenation, its frame, and (name, frame, code): every refusal that version 3 adds, each by the
    smallest edit of the valid frame, both header CRCs right wherever the check lies behind them."""
    members, widths, filters, methods = golden_set()
    x, f = b"".join(members), golden_frame()
    n, ents, table, streams = parts(f)
    count = len(ents)
    F, CK = MM.E_FORMAT, MM.E_CHECKSUM
    words = [e[2] for e in ents]

    def with_word(k, wfm):
        return M3.assemble(n, count, _entry(ents, k, word=wfm), table, streams)

    def with_table(t, ext=None, tail=b""):
        return M3.assemble(n, count, ents, t, streams + [tail], ext=ext)

    swapped = [table[1], table[0]] + table[2:]
    lo, hi = table[0] - 16, table[1] + 16
    cases = [
        ("method 2", with_word(1, M3.word(2, 0, 2)), F),
        ("method 255", with_word(0, M3.word(1, 0, 255)), F),
        ("bit 24 set", with_word(1, words[1] | 1 << 24), F),
        ("bit 31 set", with_word(3, words[3] | 1 << 31), F),
        ("no entry names a method, version 3 kept", M3.assemble(n, count, [(e[0], e[1], e[2] & 0xFFFF, e[3], e[4]) for e in ents], table, streams), F),
        ("a direct member's coded_bytes below its length", M3.assemble(n, count, _entry(ents, 2, coded=ents[2][3] - 1), table, streams), F),
        ("a table word that is no multiple of 16", with_table([table[0] + 8, table[1] - 8] + table[2:]), F),
        ("a table word below what the coder can make", with_table([M3.E.fixed_bytes(8192) + 256 * M3.E.tiles(8192) - 16,
                                                                    ents[1][0] - (M3.E.fixed_bytes(8192) + 256 * M3.E.tiles(8192) - 16)]), F),
        ("a table word above the coder's bound",
         M3.assemble(n, count, _entry(ents, 1, stream_bytes=M3.E.bound(8192) + 16 + table[1]), [M3.E.bound(8192) + 16, table[1]], streams), F),
        ("table words that do not add up to stream_bytes", with_table([table[0] + 16, table[1]]), F),
        ("a single-segment direct member's stream_bytes below the least",
         M3.assemble(n, count, _entry(ents, 2, stream_bytes=M3.E.fixed_bytes(4003) + 256 * M3.E.tiles(4003) - 16), table, streams), F),
        ("ext one pair too many", with_table(table + [0, 0], tail=b""), F),
        ("ext zero over a member with planes", with_table([], tail=bytes(16)), F),
        ("ext = 2^32 - 1", with_table(table, ext=(1 << 32) - 1), F),
        ("a table longer than the frame", with_table(table, ext=len(f) // 8), F),
        ("version 2 over a version-3 body", M3.reseal(f[:4] + b"\x02\x00\x00\x00" + f[8:]), F),
        ("version 4", M3.reseal(f[:4] + b"\x04\x00\x00\x00" + f[8:]), F),
        # canonical still: decoded through the other method's stages, in bounds
        ("a method bit cleared, others left", with_word(2, words[2] & 0xFFFF), None),
        ("a method bit set on the chain member", M3.assemble(n, count, _entry(ents, 0, word=M3.word(1, 0, 1), coded=3000), table, streams), None),
        ("two table words exchanged", with_table(swapped) if table[0] != table[1] else with_table([lo, hi]), None),
    ]
    return x, f, cases
