"""What the suites of version 2 of the member frame share (include/bwts_members.h): a member set that meets every boundary of the
delta filter beside unfiltered members, its model frame (made once), and the malformed version-2 frames with the model's codes."""
import functools

import numpy as np

import members_cases as C
import pack_members_model as MM
import pack_members_v2_model as M2
from test_pack_model import fixture_input

# (length, width, filter).  3 at width 4: shorter than an element, the identity; 9 at width 8: one element and a tail; 8193 at width 2
# and 16387 at width 4: q = 4096, a tile without elements for the tail alone; 32775 at width 8: a full tile and a tail; 4097 at width
# 1: a second tile of one element; unfiltered members of width 4, 1 and 2 between them, so that the starts are at no alignment and a
# filtered member follows an unfiltered one and the other way round.
MEMBERS = [(3, 4, 1), (8, 1, 1), (9, 8, 1), (8193, 2, 1), (4095, 4, 0), (32775, 8, 1), (4096, 1, 0), (4097, 1, 1), (16387, 4, 1), (100, 2, 0)]
LENGTHS = [m[0] for m in MEMBERS]
WIDTHS = [m[1] for m in MEMBERS]
FILTERS = [m[2] for m in MEMBERS]


def walk(ln, w, seed):
    """ln bytes of a random walk of w-byte little-endian integers with steps of a few hundred either way, from a large start: values
    whose upper bytes move, differences whose upper bytes do not."""
    rng = np.random.default_rng(seed)
    q = -(-ln // w)
    steps = rng.integers(-300, 301, q).astype(np.int64)
    a = (np.cumsum(steps) + (1 << (8 * w - 2))).astype(np.uint64)
    return a.astype({1: "u1", 2: "<u2", 4: "<u4", 8: "<u8"}[w]).tobytes()[:ln]


@functools.lru_cache(maxsize=None)
def member_set():
    """(members, widths, filters): filtered members are walks, the others text."""
    members = [walk(ln, w, 40 + k) if f else fixture_input(ln, 200 + k) for k, (ln, w, f) in enumerate(MEMBERS)]
    return members, list(WIDTHS), list(FILTERS)


@functools.lru_cache(maxsize=None)
def member_frame():
    members, widths, filters = member_set()
    return M2.pack(members, widths, filters)


def range_sets():
    """(name, ranges) over the concatenation: inside a filtered member, across a filtered/unfiltered seam either way, and the whole."""
    off = [0]
    for ln in LENGTHS:
        off.append(off[-1] + ln)
    return [
        ("inside a filtered member, far from its start", [(off[5] + 20000, 5000)]),
        ("across the seam from a filtered member into an unfiltered one", [(off[4] - 5, 10)]),
        ("across the seam from an unfiltered member into a filtered one", [(off[7] - 3, 9)]),
        ("an unfiltered member alone", [(off[6] + 1, 100)]),
        ("the short members at the front, each by a byte", [(off[k], 1) for k in range(3)]),
        ("descending, a repeat, an uncovered member between", [(off[8] + 5, 40), (off[3], 8193), (off[8] + 5, 40), (1, 2)]),
        ("whole input", [(0, off[-1])]),
    ]


SMALL_FILTERS = [1, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def small_set():
    """The four members of the version-1 malformed set (lengths 4096, 4096, 100, 9 at widths 4, 1, 2, 8), the first and the third filtered."""
    members, widths = C.small_set()
    return members, widths, list(SMALL_FILTERS)


def malformed_cases():
    """(x, f, cases): the concatenation, its valid version-2 frame, and (name, frame, code), both header CRCs right in every one."""
    members, widths, filters = small_set()
    x = b"".join(members)
    f = M2.pack(members, widths, filters)
    n, entries, _ = M2.check(f)
    count = len(entries)
    at = MM._stream_at(entries)
    streams = [f[at[k]:at[k + 1]] for k in range(count)]
    plain = MM.pack(members, widths)

    def with_words(words, version=2):
        ents = [(e[0], e[1], wf, e[3], e[4]) for e, wf in zip(entries, words)]
        return M2.assemble(n, count, ents, streams, version=version)

    words = [M2.word(w, fl) for w, fl in zip(widths, filters)]

    def one(k, wf):
        return [wf if j == k else words[j] for j in range(count)]

    F, R, CK = MM.E_FORMAT, MM.E_RANGE, MM.E_CHECKSUM
    cases = [
        ("version 1 over a version-2 body", with_words(words, version=1), F),
        ("version 3", with_words(words, version=3), F),
        ("version 2 over a version-1 body", MM.reseal(plain[:4] + b"\x02\x00\x00\x00" + plain[8:]), F),
        ("every filter cleared, version 2 kept", with_words(list(widths)), F),
        ("filter 2", with_words(one(0, M2.word(4, 2))), F),
        ("filter 255", with_words(one(1, M2.word(1, 255))), F),
        ("bit 16 set", with_words(one(0, words[0] | 1 << 16)), F),
        ("bit 31 set", with_words(one(3, words[3] | 1 << 31)), F),
        ("width byte 3 under a filter", with_words(one(2, M2.word(3, 1))), F),
        ("width byte 0 under a filter", with_words(one(2, M2.word(0, 1))), F),
        ("n = 2^32 + 1", MM.reseal(f[:8] + ((1 << 32) + 1).to_bytes(8, "little") + f[16:]), R),
        # canonical still, in bounds, and decoded through another chain than the member was packed with
        ("a filter set on an unfiltered member", with_words(one(1, M2.word(1, 1))), CK),
        ("a filter cleared, another one left", with_words(one(0, M2.word(4, 0))), CK),
        ("a filtered member's width 4 rewritten to 2", with_words(one(0, M2.word(2, 1))), CK),
    ]
    return x, f, cases
