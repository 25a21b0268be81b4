"""CPU model of the delta filter (include/bwts_delta.h): the executable form of the definition.  For a string of L bytes and a width w in
{1, 2, 4, 8}, q = L // w and a_i the little-endian unsigned elements: d_0 = a_0, d_i = a_i - a_{i-1} mod 2^{8w}; z_i = (d_i << 1) xor
(d_i >> (8w - 1), arithmetically), every element, the first one too; the L - q w bytes of the tail stay where they are; L < w is the
identity.  Decode: d_i = (z_i >> 1) xor -(z_i & 1), a_i the running sum mod 2^{8w}.  The segment form applies this to every segment
whose filter is DELTA on its own, at its own width, and copies the others."""
import numpy as np

WIDTHS = (1, 2, 4, 8)
FILTER_NONE, FILTER_DELTA = 0, 1
FILTERS = (FILTER_NONE, FILTER_DELTA)
MAX_N = 1 << 36
E = 4096                                    # the kernels' tile, in elements
COPY_T = 32768                              # the tile of a copied segment, in bytes
_DT = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}


def _u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def _check(w):
    if w not in WIDTHS:
        raise ValueError("width %r is not 1, 2, 4 or 8" % (w,))


def zigzag(d, w):
    """One difference (an integer mod 2^{8w}) to its zigzag."""
    m = (1 << (8 * w)) - 1
    d &= m
    return ((d << 1) ^ (m if d >> (8 * w - 1) else 0)) & m


def unzigzag(z, w):
    m = (1 << (8 * w)) - 1
    return ((z >> 1) ^ (m if z & 1 else 0)) & m


def encode(x, w):
    _check(w)
    x = _u8(x)
    q = x.size // w
    a = x[:q * w].view(_DT[w])
    d = a.copy()
    d[1:] = a[1:] - a[:-1]                  # (unsigned numpy arithmetic wraps mod 2^{8w})
    z = (d << 1) ^ np.negative(d >> (8 * w - 1))                    # (minus the sign bit: all ones where the difference is negative)
    return np.concatenate((z.astype(_DT[w]).view(np.uint8), x[q * w:]))


def decode(y, w):
    _check(w)
    y = _u8(y)
    q = y.size // w
    z = y[:q * w].view(_DT[w])
    d = (z >> 1) ^ np.negative(z & 1)
    a = np.cumsum(d, dtype=_DT[w])
    return np.concatenate((a.astype(_DT[w]).view(np.uint8), y[q * w:]))


def _segments(f, x, lengths, widths, filters):
    x = _u8(x)
    assert sum(int(v) for v in lengths) == x.size and all(int(v) > 0 for v in lengths) and len(widths) == len(lengths) == len(filters)
    out, at = [], 0
    for ln, w, flt in zip(lengths, widths, filters):
        _check(w)
        if flt not in FILTERS:
            raise ValueError("filter %r is not 0 or 1" % (flt,))
        seg = x[at:at + int(ln)]
        out.append(f(seg, w) if flt == FILTER_DELTA else seg)
        at += int(ln)
    return np.concatenate(out)


def encode_segments(x, lengths, widths, filters):
    return _segments(encode, x, lengths, widths, filters)


def decode_segments(y, lengths, widths, filters):
    return _segments(decode, y, lengths, widths, filters)


def tiles(ln, w, flt):
    """The tiles the kernels give a segment."""
    t = E * w if flt == FILTER_DELTA else COPY_T
    return -(-ln // t)
