"""CPU model of the move-to-front stage (include/bwts_mtf.h): the serial definition, its segmented form, and the tiled
formulation the device runs -- a scan over 256-byte list states with two associative, non-commutative operators and a reset at
every segment start.  The tiled functions are the executable statement of the state algebra (bijective-bwt_amd/csrc/mtf.hip)."""
import numpy as np

IDENTITY = bytes(range(256))


# -- the definition ------------------------------------------------------------------------
def forward(data):
    lst = bytearray(IDENTITY)
    out = bytearray(len(data))
    for i, c in enumerate(bytes(data)):
        k = lst.index(c)
        out[i] = k
        del lst[k]
        lst.insert(0, c)
    return bytes(out)


def inverse(data):
    lst = bytearray(IDENTITY)
    out = bytearray(len(data))
    for i, k in enumerate(bytes(data)):
        c = lst[k]
        out[i] = c
        del lst[k]
        lst.insert(0, c)
    return bytes(out)


def segmented(fn, data, lengths):
    """fn on every segment alone: the list starts afresh at every segment."""
    data = bytes(data)
    assert sum(int(x) for x in lengths) == len(data)
    out, at = [], 0
    for ln in lengths:
        out.append(fn(data[at:at + int(ln)]))
        at += int(ln)
    return b"".join(out)


# -- the tiled formulation -------------------------------------------------------------------
def cut(lengths, T):
    """Tiles of at most T bytes, none across a segment start: (begin, end, starts_a_segment)."""
    tiles, at = [], 0
    for ln in lengths:
        ln = int(ln)
        for a in range(at, at + ln, T):
            tiles.append((a, min(a + T, at + ln), a == at))
        at += ln
    return tiles


def _run_from(lst, data):
    """Forward MTF over data from the list lst: (ranks, list afterwards)."""
    lst = bytearray(lst)
    out = bytearray(len(data))
    for i, c in enumerate(data):
        k = lst.index(c)
        out[i] = k
        del lst[k]
        lst.insert(0, c)
    return bytes(out), bytes(lst)


def forward_state(tile):
    """(list after MTF over the tile from the identity, number of distinct symbols seen): the seen symbols stand in front, the most
    recent first, the others behind in ascending order."""
    _, lst = _run_from(IDENTITY, tile)
    return lst, len(set(tile))


def forward_compose(a, b):
    """A then B = B.list[0 .. d_B) followed by the symbols of A.list that B has not seen, in A.list's order; d = size of the union."""
    (la, da), (lb, db) = a, b
    seen = set(lb[:db])
    rest = bytes(s for s in la if s not in seen)
    return lb[:db] + rest, db + sum(1 for s in la[:da] if s not in seen)


def inverse_state(tile):
    """The tile's ranks decoded on placeholders 0 .. 255: (placeholder index per position, final permutation pi with end[k] = start[pi[k]])."""
    lst = bytearray(IDENTITY)
    idx = bytearray(len(tile))
    for i, k in enumerate(tile):
        p = lst[k]
        idx[i] = p
        del lst[k]
        lst.insert(0, p)
    return bytes(idx), bytes(lst)


def inverse_compose(a, b):
    """(A then B)[k] = A[B[k]]."""
    return bytes(a[k] for k in b)


def exclusive_scan(states, resets, compose, identity):
    """The running prefix in front of every state; a reset puts the identity there, and the state behind it stands alone."""
    out, acc = [], identity
    for st, r in zip(states, resets):
        out.append(identity if r else acc)
        acc = st if r else compose(acc, st)
    return out


def forward_tiled(data, T, lengths=None):
    data = bytes(data)
    tiles = cut([len(data)] if lengths is None else lengths, T)
    states = [forward_state(data[a:b]) for a, b, _ in tiles]
    starts = exclusive_scan(states, [r for _, _, r in tiles], forward_compose, (IDENTITY, 0))
    return b"".join(_run_from(st[0], data[a:b])[0] for (a, b, _), st in zip(tiles, starts))


def inverse_tiled(data, T, lengths=None):
    data = bytes(data)
    tiles = cut([len(data)] if lengths is None else lengths, T)
    parts = [inverse_state(data[a:b]) for a, b, _ in tiles]
    starts = exclusive_scan([p[1] for p in parts], [r for _, _, r in tiles], inverse_compose, IDENTITY)
    return b"".join(bytes(st[i] for i in idx) for (idx, _), st in zip(parts, starts))


# -- the same two loops at numpy speed, for the GPU suite's larger cases (checked against the definition in test_mtf_model.py) ------
def forward_fast(data):
    """forward() with the rank-0 bytes (a symbol equal to its predecessor) skipped at numpy speed."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(a.size, dtype=np.uint8)
    if a.size == 0:
        return out.tobytes()
    heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    lst = bytearray(IDENTITY)
    for i, c in zip(heads.tolist(), a[heads].tolist()):
        k = lst.index(c)
        out[i] = k
        if k:
            del lst[k]
            lst.insert(0, c)
    return out.tobytes()


def inverse_fast(data):
    """inverse() with the zero ranks filled in at numpy speed: such a position repeats the symbol in front of it."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(a.size, dtype=np.uint8)
    nz = np.flatnonzero(a)
    lst = bytearray(IDENTITY)
    sym = np.empty(nz.size + 1, dtype=np.uint8)
    sym[0] = 0                      # before the first nonzero rank the front is the identity's: symbol 0
    for j, k in enumerate(a[nz].tolist()):
        c = lst[k]
        del lst[k]
        lst.insert(0, c)
        sym[j + 1] = c
    which = np.cumsum(a != 0)       # nonzero ranks at or before each position
    out[:] = sym[which]
    return out.tobytes()
