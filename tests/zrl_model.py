"""CPU model of the zero-run stage (include/bwts_zrl.h): the coded form in plain numpy -- encode (coded or stored), decode (None for a
malformed input, with the reason in why()), the segment forms, and the malformed inputs the decoders must refuse."""
import numpy as np

MAX_DIGITS = 36
MAX_N = 1 << 36
E_FORMAT = -8
BAD_PAYLOAD, BAD_DIGIT, BAD_END, BAD_SUM, TOO_LONG = "payload", "digit", "end", "sum", "longer than n"


def _u8(x):
    return x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), dtype=np.uint8)


def run_digits(L):
    """The digit bytes of a run of L >= 1 zeros: bijective base 2, least significant first."""
    out = []
    while L:
        d = (L - 1) & 1
        out.append(d)
        L = (L - 1 - d) >> 1
    return out


def coded(r):
    """The m bytes the ranks become, whether or not they are fewer than the ranks (bytes)."""
    r = _u8(r)
    n = r.size
    nz = np.flatnonzero(r)
    vals = r[nz].astype(np.int64)
    gaps = np.diff(np.concatenate(([-1], nz, [n]))).astype(np.int64) - 1      # zeros in front of every rank that is not 0, and behind the last
    k = np.where(gaps > 0, np.frexp((gaps + 1).astype(np.float64))[1] - 1, 0).astype(np.int64)      # floor(log2(L + 1)), exact below 2^53
    wide = vals >= 254
    sizes = np.zeros(2 * vals.size + 1, dtype=np.int64)        # run, rank, run, rank, ..., run
    sizes[0::2] = k
    sizes[1::2] = np.where(wide, 2, 1)
    offs = np.concatenate(([0], np.cumsum(sizes)))
    out = np.zeros(int(offs[-1]), dtype=np.uint8)
    lo = offs[1:-1:2]
    out[lo] = np.where(wide, 255, vals + 1)
    out[lo[wide] + 1] = vals[wide] - 254
    go = offs[0:-1:2]
    for i in range(int(k.max()) if k.size else 0):
        sel = k > i
        out[go[sel] + i] = ((gaps[sel] + 1) >> i) & 1
    return out.tobytes()


def coded_serial(r):
    """coded() as the header states it, rank by rank: what the vectorised form is held against."""
    out, L = bytearray(), 0
    for v in _u8(r).tolist():
        if v == 0:
            L += 1
            continue
        out += bytes(run_digits(L))
        L = 0
        out += bytes([255, v - 254]) if v >= 254 else bytes([v + 1])
    return bytes(out + bytes(run_digits(L)))


def encode(r):
    """What the stage writes for r: the coded bytes where they are fewer than the ranks, else the ranks themselves."""
    r = _u8(r)
    assert r.size >= 1
    z = coded(r)
    return z if len(z) < r.size else r.tobytes()


_why = [None]


def why():
    return _why[0]


def _refuse(reason):
    _why[0] = reason
    return None


def decode(z, n):
    """The n ranks that z stands for, or None where the decoder must answer BWTS_E_FORMAT (why() names the first reason found)."""
    z = _u8(z)
    n = int(n)
    _why[0] = None
    if z.size == n:
        return z.tobytes()
    if z.size > n:
        return _refuse(TOO_LONG)
    lits = []
    pos, i, p = 0, 0, 0
    zl = z.tolist()
    while p < len(zl):
        b = zl[p]
        if b == 255:
            if p + 1 == len(zl):
                return _refuse(BAD_END)
            if zl[p + 1] > 1:
                return _refuse(BAD_PAYLOAD)
            lits.append((pos, 254 + zl[p + 1]))
            pos += 1
            i = 0
            p += 2
            continue
        if b <= 1:
            if i >= MAX_DIGITS:
                return _refuse(BAD_DIGIT)
            pos += (b + 1) << i
            i += 1
        else:
            lits.append((pos, b - 1))
            pos += 1
            i = 0
        p += 1
        if pos > n:
            return _refuse(BAD_SUM)
    if pos != n:
        return _refuse(BAD_SUM)
    out = np.zeros(n, dtype=np.uint8)          # (only now: a refused input may name 2^36 ranks)
    if lits:
        at, v = zip(*lits)
        out[np.array(at, dtype=np.int64)] = np.array(v, dtype=np.uint8)
    return out.tobytes()


def encode_segments(r, lengths):
    r = _u8(r)
    out, at = [], 0
    for ln in lengths:
        out.append(encode(r[at:at + int(ln)]))
        at += int(ln)
    assert at == r.size
    return out


def decode_segments(z, in_lengths, lengths):
    z = _u8(z)
    out, at = [], 0
    for il, ln in zip(in_lengths, lengths):
        d = decode(z[at:at + int(il)], ln)
        if d is None:
            return None
        out.append(d)
        at += int(il)
    return b"".join(out)


def malformed_cases():
    """(name, z, n): inputs every decoder refuses with BWTS_E_FORMAT.  good stands for 11 ranks: 4, five zeros, 2, 255, three zeros."""
    good = bytes([5, 0, 1, 3, 255, 1, 0, 0])
    n = len(decode_ok(good))
    return [
        ("in_bytes > n", bytes([2, 3, 4, 5]), 3),
        ("sum n - 1", good, n + 1),
        ("sum n + 1", good, n - 1),
        ("255 at the end", bytes([5, 0, 255]), 40),
        ("255 followed by 2", bytes([5, 255, 2, 0, 0]), 40),
        ("40 digits in a row", bytes([7] + [0] * 40 + [9]), 4096),
        ("40 digits in a row, n = 2^36", bytes([7] + [0] * 40 + [9]), 1 << 36),
        ("digit of index 35, n = 100", bytes([0] * 36), 100),
    ]


def decode_ok(z):
    """The ranks of a well-formed coded input whose n is not known: a test helper that walks the same rules."""
    z = _u8(z).tolist()
    pos, i, p = 0, 0, 0
    lits = []
    while p < len(z):
        b = z[p]
        if b == 255:
            lits.append((pos, 254 + z[p + 1]))
            pos, i, p = pos + 1, 0, p + 2
            continue
        if b <= 1:
            pos += (b + 1) << i
            i += 1
        else:
            lits.append((pos, b - 1))
            pos, i = pos + 1, 0
        p += 1
    out = np.zeros(pos, dtype=np.uint8)
    for at, v in lits:
        out[at] = v
    return out.tobytes()
