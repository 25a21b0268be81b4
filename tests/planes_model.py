"""CPU model of the byte-plane split (include/bwts_planes.h): the executable form of the definition.  For a string of L bytes and a
width w in {2, 4, 8}, q = L // w: out[k q + i] = in[i w + k], the L - q w bytes of the tail stay where they are; L < w is the identity.
The segment form applies this to every segment on its own."""
import numpy as np

WIDTHS = (2, 4, 8)
MAX_N = 1 << 36
E = 4096                                    # the kernels' tile, in elements


def _u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, dtype=np.uint8)


def _check(w):
    if w not in WIDTHS:
        raise ValueError("width %r is not 2, 4 or 8" % (w,))


def split(x, w):
    _check(w)
    x = _u8(x)
    q = x.size // w
    return np.concatenate((x[:q * w].reshape(q, w).T.reshape(-1), x[q * w:]))


def join(y, w):
    _check(w)
    y = _u8(y)
    q = y.size // w
    return np.concatenate((y[:q * w].reshape(w, q).T.reshape(-1), y[q * w:]))


def _segments(f, x, lengths, w):
    x = _u8(x)
    assert sum(int(v) for v in lengths) == x.size and all(int(v) > 0 for v in lengths)
    out, at = [], 0
    for ln in lengths:
        out.append(f(x[at:at + int(ln)], w))
        at += int(ln)
    return np.concatenate(out)


def split_segments(x, lengths, w):
    return _segments(split, x, lengths, w)


def join_segments(y, lengths, w):
    return _segments(join, y, lengths, w)


def plan(n, w):
    """What bwts_debug_planes_plan answers: the tile in bytes, the tiles, the whole elements and the tail's bytes."""
    _check(w)
    return {"T": E * w, "tiles": -(-n // (E * w)), "q": n // w, "tail": n - n // w * w}
