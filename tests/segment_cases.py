"""Structured segment sets for the segmented transforms (tests/test_segments.py) and their expected output from the CPU oracle.

Every builder is seeded and returns (data: uint8 array, lengths: uint64 array).  Unlike random segmentations, these sets share
material between segments: copies of a few documents, near copies, records with one shared header, overlapping windows of one
text, powers of Lyndon words.  So groups of equal infinite words span many segments, and the stable partition of the shared pass
has to put each group's bytes into the right segments.

The expected output is computed once per distinct segment content (the sets repeat content a lot) and assembled; segments stay
short (at most 128 KiB, except the one long segment of the mixed-route case), since the oracle is quadratic on long runs.
"""
import numpy as np

import oracle_lib as O

SEG_FWD_BIG = 2 << 20          # from this length a segment takes the single-input forward on its own (csrc/forward.hip)


def _pack(segs):
    segs = [np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s for s in segs]
    return np.concatenate(segs), np.array([s.size for s in segs], dtype=np.uint64)


def _bounds(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=off[1:])
    return off


def split(data, lengths):
    off = _bounds(lengths)
    return [data[off[i]:off[i + 1]] for i in range(len(lengths))]


def _docs(rng, ndocs, doc_len, kinds=("text", "zipf")):
    return [O.generate(kinds[i % len(kinds)], doc_len, int(rng.integers(1 << 30))) for i in range(ndocs)]


# ---- families ----------------------------------------------------------------------------------------------------------------------

def copies(seed, doc_len, r, ndocs=3):
    """ndocs documents, each repeated r times, in shuffled order: r equal infinite words per position of a document."""
    rng = np.random.default_rng(seed)
    docs = _docs(rng, ndocs, doc_len)
    order = rng.permutation(np.repeat(np.arange(ndocs), r))
    return _pack([docs[i] for i in order])


def near_copies(seed, doc_len, r, ndocs=2):
    """Like copies, with one or two bytes of every copy edited at random places: groups split late, deep in the rounds."""
    rng = np.random.default_rng(seed)
    docs = _docs(rng, ndocs, doc_len)
    segs = []
    for i in rng.permutation(np.repeat(np.arange(ndocs), r)):
        c = docs[i].copy()
        for p in rng.integers(0, doc_len, int(rng.integers(1, 3))):
            c[p] = (int(c[p]) + int(rng.integers(1, 256))) & 0xFF
        segs.append(c)
    return _pack(segs)


def records(seed, count, header_len, tail_lo=16, tail_hi=256):
    """One shared header of header_len bytes, then a distinct tail of tail_lo .. tail_hi bytes per record."""
    rng = np.random.default_rng(seed)
    header = O.generate("text", header_len, int(rng.integers(1 << 30)))
    tails = O.generate("zipf", count * tail_hi, int(rng.integers(1 << 30)))
    segs = []
    for i in range(count):
        t = int(rng.integers(tail_lo, tail_hi + 1))
        segs.append(np.concatenate([header, tails[i * tail_hi:i * tail_hi + t]]))
    return _pack(segs)


def windows(seed, L, step, count, kind="text"):
    """Windows of length L of one text at offsets i * step (step < L): neighbours share L - step bytes."""
    assert 0 < step < L
    rng = np.random.default_rng(seed)
    src = O.generate(kind, (count - 1) * step + L, int(rng.integers(1 << 30)))
    win = np.lib.stride_tricks.sliding_window_view(src, L)[::step][:count]
    return np.ascontiguousarray(win).reshape(-1), np.full(count, L, dtype=np.uint64)


LYNDON_WORDS = [b"ab", b"abb", b"aab", b"aabab", b"abc", b"\x00a\xff", b"aabaabb"]


def periodic(seed, words=LYNDON_WORDS, per_word=300, kmax=1500):
    """u^k and u^k.v (v a proper prefix of u) for Lyndon words u and many k."""
    rng = np.random.default_rng(seed)
    segs = []
    for u in words:
        for k in rng.integers(1, kmax + 1, per_word):
            segs.append(u * int(k))
            segs.append(u * int(k) + u[:int(rng.integers(1, len(u)))])
    order = rng.permutation(len(segs))
    return _pack([segs[i] for i in order])


def periodic_one(seed, u, total, kmax=4096):
    """(u)^k for random k up to kmax until about `total` bytes: every position stays tied to the end, and equal factors sit in
    thousands of segments."""
    rng = np.random.default_rng(seed)
    ks, left = [], total // len(u)
    while left > 0:
        k = int(min(left, rng.integers(1, kmax + 1)))
        ks.append(k)
        left -= k
    return _pack([u * k for k in ks])


def powers(seed, wlen=300, kmax=100):
    """w, w^2, ..., w^kmax and every rotation of w, shuffled."""
    rng = np.random.default_rng(seed)
    w = bytes(O.generate("text", wlen, int(rng.integers(1 << 30))))
    segs = [w * k for k in range(1, kmax + 1)] + [w[i:] + w[:i] for i in range(wlen)]
    return _pack([segs[i] for i in rng.permutation(len(segs))])


def constant(seed, total=2 << 20, hi=4000, value=ord("q")):
    """Every segment the same byte value, of random lengths: the constant-input shortcut of the forward."""
    rng = np.random.default_rng(seed)
    ls, left = [], total
    while left:
        n = int(min(left, rng.integers(1, hi + 1)))
        ls.append(n)
        left -= n
    return np.full(total, value, dtype=np.uint8), np.array(ls, dtype=np.uint64)


def mixed_route(seed, doc_len=4096, r=300, long_len=(2 << 20) + 12345):
    """copies of two documents, plus one segment of more than 2 MiB made of the same documents (which takes the single-input route)
    placed in the middle."""
    rng = np.random.default_rng(seed)
    docs = _docs(rng, 2, doc_len)
    segs = [docs[i] for i in rng.permutation(np.repeat(np.arange(2), r))]
    reps = long_len // doc_len + 1
    long_seg = np.concatenate([docs[int(i)] for i in rng.integers(0, 2, reps)])[:long_len]
    segs.insert(len(segs) // 2, long_seg)
    return _pack(segs)


# name -> (builder, minimum `rounds` of the forward, or None when the family is not meant to tie).  The minima are one below what the
# cases measured (periodic sets: every group is one of equal infinite words after round 0, so the first list round splits nothing).
FAMILIES = {
    "copies_16k_x200": (lambda: copies(101, 16 << 10, 200), 6),      # groups of 200: LDS counting
    "copies_4k_x1000": (lambda: copies(102, 4 << 10, 1000), 5),      # groups of 1000: WIDE chunks
    "copies_1k_x3000": (lambda: copies(103, 1 << 10, 3000), 4),      # groups of 3000: the big list
    "copies_100_x20000": (lambda: copies(104, 100, 20000), 3),       # groups of 20 000
    "near_copies_4k": (lambda: near_copies(105, 4 << 10, 600), 6),
    "near_copies_1k": (lambda: near_copies(106, 1 << 10, 3000), 5),
    "records": (lambda: records(107, 2000, 6000), 6),
    "windows_8k_step1000": (lambda: windows(108, 8192, 1000, 1500), 7),
    "windows_2k_step7": (lambda: windows(109, 2048, 7, 4000), 6),
    "periodic": (lambda: periodic(110), 2),
    "periodic_ab_16m": (lambda: periodic_one(111, b"ab", 16 << 20), 2),
    "periodic_abb_16m": (lambda: periodic_one(112, b"abb", 16 << 20), 2),
    "powers": (lambda: powers(113), 5),
    "constant": (lambda: constant(114), None),
    "mixed_route": (lambda: mixed_route(115), 9),
}


def build(name):
    return FAMILIES[name][0]()


# ---- expected output --------------------------------------------------------------------------------------------------------------

def _by_content(fn, data, lengths):
    cache = {}
    out = np.empty_like(data)
    off = _bounds(lengths)
    for i in range(len(lengths)):
        a, b = int(off[i]), int(off[i + 1])
        key = data[a:b].tobytes()
        y = cache.get(key)
        if y is None:
            y = cache[key] = fn(data[a:b])
        out[a:b] = y
    return out


def expected_forward(data, lengths):
    return _by_content(O.forward, data, lengths)


def expected_inverse(data, lengths):
    return _by_content(O.inverse, data, lengths)


def expected_factors(data, lengths):
    """The number of Lyndon factors summed over the segments (each segment factorised on its own)."""
    cache = {}
    total = 0
    off = _bounds(lengths)
    for i in range(len(lengths)):
        key = data[int(off[i]):int(off[i + 1])].tobytes()
        c = cache.get(key)
        if c is None:
            c = cache[key] = len(O.lyndon_starts(np.frombuffer(key, dtype=np.uint8)))
        total += c
    return total


# ---- many tiny segments: expected output by lookup table ------------------------------------------------------------------------------

TINY_ALPHABET = np.array([0x00, 0x01, 0x61, 0x62, 0xFE, 0xFF], dtype=np.uint8)


def partition_passes(count):
    """LSD passes of 8 bits the stable partition of the forward runs over the segment id (partition_by_segment)."""
    bits = max(1, int(count - 1).bit_length())
    return (bits + 7) // 8


def tiny_segments(seed, count, alphabet=TINY_ALPHABET):
    """count segments of 1 .. 3 bytes over a small alphabet (0x00 and 0xff included)."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 4, count).astype(np.uint64)
    data = alphabet[rng.integers(0, alphabet.size, int(lengths.sum()))]
    return data, lengths


class TinyTable:
    """The oracle on every word of length 1 .. 3 over `alphabet` (a few hundred entries), applied to a whole segment set with vectorised
    numpy: no Python loop over segments."""

    def __init__(self, fn, alphabet=TINY_ALPHABET):
        self.alphabet = alphabet
        self.code = np.full(256, -1, dtype=np.int64)
        self.code[alphabet] = np.arange(alphabet.size)
        A = alphabet.size
        self.out, self.factors = {}, {}
        for L in (1, 2, 3):
            words = np.array(np.unravel_index(np.arange(A ** L), (A,) * L)).T       # row c: the digits of code c, most significant first
            self.out[L] = np.stack([fn(alphabet[w]) for w in words])
            self.factors[L] = np.array([len(O.lyndon_starts(alphabet[w])) for w in words], dtype=np.int64)

    def _classes(self, data, lengths):
        off = _bounds(lengths)[:-1]
        ls = np.asarray(lengths, dtype=np.int64)
        A = self.alphabet.size
        for L in (1, 2, 3):
            starts = off[ls == L]
            if not starts.size:
                continue
            pos = starts[:, None] + np.arange(L)[None, :]
            digits = self.code[data[pos]]
            assert (digits >= 0).all(), "byte outside the table's alphabet"
            code = np.zeros(starts.size, dtype=np.int64)
            for j in range(L):
                code = code * A + digits[:, j]
            yield L, pos, code

    def apply(self, data, lengths):
        assert int(np.asarray(lengths).max()) <= 3
        out = np.empty_like(data)
        for L, pos, code in self._classes(data, lengths):
            out[pos] = self.out[L][code]
        return out

    def count_factors(self, data, lengths):
        return int(sum(self.factors[L][code].sum() for L, _, code in self._classes(data, lengths)))
