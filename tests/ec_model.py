"""CPU model of the entropy coder (include/bwts_ec.h): the version-1 stream in plain numpy -- encode, decode (None for a malformed
stream), the bound, and the segment forms.  It is the executable statement of the format: the device code (bijective-bwt_amd/csrc/ec.hip)
must produce these bytes, and must refuse what decode() refuses.

The 64 lanes of a tile run as one numpy row, and many tiles as the rows of one array, so a step of the coder is a handful of array
operations whatever the input's size."""
import numpy as np

LOG_T, LOG_K, PROB_BITS = 14, 4, 12
T, K, M = 1 << LOG_T, 1 << LOG_K, 1 << PROB_BITS
L = 1 << 16
ROW = 1024
MAGIC = 0x43455742
PARAMS = LOG_T | LOG_K << 8 | PROB_BITS << 16
MAX_N = 1 << 36
CHUNK = 256                      # tiles coded side by side

_LANE = np.arange(64, dtype=np.int64)


def pad16(x):
    return (x + 15) & ~15


def tiles(n):
    return (n + T - 1) // T


def blocks(nt):
    return (nt + K - 1) // K


def fixed_bytes(n):
    nt = tiles(n)
    return 16 + 512 * blocks(nt) + pad16(4 * nt)


def bound(n):
    return fixed_bytes(n) + 272 * tiles(n) + 2 * n


def bound_segments(lengths):
    return sum(bound(int(x)) for x in lengths)


def normalise(h):
    """256 byte counts -> 256 frequencies summing to 4096 (the rule of the stream's tables, in its order)."""
    h = np.asarray(h, dtype=np.int64)
    m = int(h.sum())
    f = np.where(h > 0, np.maximum(1, h * M // m), 0)
    d = M - int(f.sum())
    if d > 0:
        f[int(np.argmax(f))] += d          # (argmax: the first of equals, the lowest symbol)
    while d < 0:
        f[int(np.argmax(f))] -= 1
        d += 1
    return f


def cross_entropy_bits(data):
    """X of the issue: sum over the blocks of h[s] log2(4096 / f[s]), the cost of the input under the stored tables."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    bits = 0.0
    for at in range(0, a.size, K * T):
        h = np.bincount(a[at:at + K * T], minlength=256)
        f = normalise(h)
        nz = h > 0
        bits += float((h[nz] * np.log2(M / f[nz])).sum())
    return bits


# -- the coder proper, over the rows of an array of tiles ------------------------------------------
def _encode_tiles(data, lens, f, c):
    """data: (C, T) uint8, zero behind each tile's end; lens: (C,); f, c: (C, 256) tables of each tile's block.
    -> (final states (C, 64) uint32, every tile's words in the decoder's order, concatenated; words per tile (C,)).
    States are uint32 here, so x >= f 2^20 is written as f < 4096 and x >= (f << 20 mod 2^32): the 64-bit comparison of the format."""
    C = data.shape[0]
    rows = int((int(lens.max()) + ROW - 1) // ROW)
    S = 16 * rows
    d4 = data.reshape(C, T // ROW, 64, 16)                   # [tile, row, lane, byte of the lane's 16]
    tab = (f | c << 16).astype(np.uint32).ravel()             # f and c of one symbol in one gather
    base = (256 * np.arange(C, dtype=np.intp))[:, None]
    x = np.full((C, 64), L, dtype=np.uint32)
    mask = np.zeros((C, S, 64), dtype=bool)
    vals = np.zeros((C, S, 64), dtype=np.uint16)
    ln = lens.astype(np.int64)[:, None]
    full = int(lens.min())
    for j in range(S - 1, -1, -1):
        r, k = j >> 4, j & 15
        e = tab[d4[:, r, :, k] + base]
        fs, cs = e & np.uint32(0xFFFF), e >> np.uint32(16)
        emit = (fs < np.uint32(M)) & (x >= (fs << np.uint32(20)))
        active = None
        if (r + 1) * ROW > full:
            active = (r * ROW + _LANE * 16 + k)[None, :] < ln
            emit &= active
        mask[:, j] = emit
        vals[:, j] = x                                         # (the low 16 bits)
        x = np.where(emit, x >> np.uint32(16), x)
        fd = np.maximum(fs, np.uint32(1))
        q = x // fd
        xn = q * np.uint32(M) + (x - q * fd) + cs
        x = xn if active is None else np.where(active, xn, x)
    assert int(x.min()) >= L
    return x, vals[mask], mask.sum(axis=(1, 2))


def _tables(a, lengths):
    """Per block of every segment: the frequencies (NB, 256); and per tile its block's index."""
    fs, tile_block = [], []
    at = 0
    for ln in lengths:
        for b0 in range(at, at + ln, K * T):
            b1 = min(b0 + K * T, at + ln)
            tile_block += [len(fs)] * tiles(b1 - b0)
            fs.append(normalise(np.bincount(a[b0:b1], minlength=256)))
        at += ln
    return np.array(fs, dtype=np.int64).reshape(-1, 256), np.array(tile_block, dtype=np.int64)


def encode_segments(data, lengths):
    """One stream per segment, each what encode() gives for the segment alone."""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    lengths = [int(x) for x in lengths]
    assert lengths and min(lengths) >= 1 and sum(lengths) == a.size
    F, tile_block = _tables(a, lengths)
    Cx = np.cumsum(F, axis=1) - F
    nt_all = tile_block.size
    lens = np.empty(nt_all, dtype=np.int64)
    starts = np.empty(nt_all, dtype=np.int64)
    t, at = 0, 0
    for ln in lengths:
        nt = tiles(ln)
        starts[t:t + nt] = at + T * np.arange(nt)
        lens[t:t + nt] = T
        lens[t + nt - 1] = ln - T * (nt - 1)
        t += nt
        at += ln
    states, words, counts = [], [], []
    padded = np.concatenate((a, np.zeros(T, dtype=np.uint8)))
    for c0 in range(0, nt_all, CHUNK):
        c1 = min(c0 + CHUNK, nt_all)
        d = padded[starts[c0:c1, None] + np.arange(T)[None, :]]
        d[np.arange(T)[None, :] >= lens[c0:c1, None]] = 0
        st, w, cnt = _encode_tiles(d, lens[c0:c1], F[tile_block[c0:c1]], Cx[tile_block[c0:c1]])
        states.append(st); words.append(w); counts.append(cnt)
    states, words, counts = np.concatenate(states), np.concatenate(words), np.concatenate(counts).astype(np.int64)
    wat = np.concatenate(([0], np.cumsum(counts)))
    sizes = (256 + 2 * counts + 15) & ~15
    out, t, b = [], 0, 0
    for ln in lengths:
        nt, nb = tiles(ln), blocks(tiles(ln))
        parts = [np.array([MAGIC, PARAMS, ln & 0xFFFFFFFF, ln >> 32], dtype="<u4").tobytes(),
                 F[b:b + nb].astype("<u2").tobytes()]
        dirb = sizes[t:t + nt].astype("<u4").tobytes()
        parts.append(dirb + bytes(pad16(len(dirb)) - len(dirb)))
        for i in range(t, t + nt):
            pay = states[i].astype("<u4").tobytes() + words[wat[i]:wat[i + 1]].astype("<u2").tobytes()
            parts.append(pay + bytes(int(sizes[i]) - len(pay)))
        out.append(b"".join(parts))
        t += nt
        b += nb
    return out


def encode(data):
    data = bytes(data) if not isinstance(data, np.ndarray) else data
    return encode_segments(data, [len(data)])[0]


def _decode_tiles(states, words, nwords, sizes, lens, symtab, f, c):
    """states (C, 64); words (C, W) uint16, zero behind each tile's own; nwords: the words each payload holds, padding included;
    sizes: payload bytes; symtab (C, 4096): slot -> symbol; f, c (C, 256).  -> (bytes (C, T), ok (C,))."""
    C = states.shape[0]
    S = 16 * int((int(lens.max()) + ROW - 1) // ROW)
    x = states.astype(np.uint64)
    out = np.zeros((C, T), dtype=np.uint8)
    rp = np.zeros(C, dtype=np.int64)
    bad = np.zeros(C, dtype=bool)
    ln = lens.astype(np.int64)[:, None]
    W = words.shape[1]
    for j in range(S):
        p = (j >> 4) * ROW + _LANE * 16 + (j & 15)
        active = p[None, :] < ln
        slot = (x & np.uint64(M - 1)).astype(np.int64)
        s = np.take_along_axis(symtab, slot, axis=1)
        fs = np.take_along_axis(f, s, axis=1).astype(np.uint64)
        cs = np.take_along_axis(c, s, axis=1).astype(np.uint64)
        x = np.where(active, fs * (x >> np.uint64(PROB_BITS)) + slot.astype(np.uint64) - cs, x)
        out[:, p] = np.where(active, s, 0).astype(np.uint8)
        need = active & (x < np.uint64(L))
        idx = rp[:, None] + np.cumsum(need, axis=1) - 1
        over = need & (idx >= nwords[:, None])
        bad |= over.any(axis=1)
        w = np.take_along_axis(words, np.clip(idx, 0, W - 1), axis=1).astype(np.uint64)
        x = np.where(need & ~over, (x << np.uint64(16)) | w, x)
        rp += need.sum(axis=1)
    ok = ~bad & (x == np.uint64(L)).all(axis=1) & (rp <= nwords) & (((256 + 2 * rp + 15) & ~15) == sizes)
    tail = np.arange(W)[None, :] >= rp[:, None]
    ok &= ~((words != 0) & tail).any(axis=1)
    return out, ok


def _parse(stream, want_n=None):
    """Everything in front of the payloads: (n, F (nb, 256), payload offsets (nt + 1) from the stream's start) or None."""
    if len(stream) < 16 or len(stream) % 16:
        return None
    magic, params, lo, hi = np.frombuffer(stream[:16], dtype="<u4").tolist()
    n = lo | hi << 32
    if magic != MAGIC or params != PARAMS or n == 0 or n > MAX_N or (want_n is not None and n != want_n):
        return None
    nt, nb = tiles(n), blocks(tiles(n))
    fixed = fixed_bytes(n)
    if len(stream) < fixed + 256 * nt or len(stream) > bound(n):
        return None
    F = np.frombuffer(stream[16:16 + 512 * nb], dtype="<u2").astype(np.int64).reshape(nb, 256)
    if (F.sum(axis=1) != M).any():
        return None
    dirb = stream[16 + 512 * nb:fixed]
    sizes = np.frombuffer(dirb[:4 * nt], dtype="<u4").astype(np.int64)
    if any(dirb[4 * nt:]):
        return None
    lens = np.full(nt, T, dtype=np.int64)
    lens[-1] = n - T * (nt - 1)
    if (sizes < 256).any() or (sizes % 16).any() or (sizes > ((256 + 2 * lens + 15) & ~15)).any():
        return None
    if fixed + int(sizes.sum()) != len(stream):
        return None
    return n, F, fixed + np.concatenate(([0], np.cumsum(sizes))), lens


def decode(stream, want_n=None):
    """The bytes of a version-1 stream, or None when it is malformed (want_n: the length the header must name)."""
    stream = bytes(stream)
    parsed = _parse(stream, want_n)
    if parsed is None:
        return None
    n, F, offs, lens = parsed
    nt = lens.size
    Cx = np.cumsum(F, axis=1) - F
    symtab = np.stack([np.repeat(np.arange(256, dtype=np.int64), row) for row in F])
    raw = np.frombuffer(stream, dtype=np.uint8)
    pieces = []
    for c0 in range(0, nt, CHUNK):
        c1 = min(c0 + CHUNK, nt)
        sizes = offs[c0 + 1:c1 + 1] - offs[c0:c1]
        nwords = (sizes - 256) // 2
        W = max(int(nwords.max()), 1)
        states = np.stack([raw[offs[i]:offs[i] + 256].view("<u4") for i in range(c0, c1)])
        words = np.zeros((c1 - c0, W), dtype=np.uint16)
        for i in range(c0, c1):
            words[i - c0, :nwords[i - c0]] = raw[offs[i] + 256:offs[i + 1]].view("<u2")
        blk = np.arange(c0, c1) // K
        out, ok = _decode_tiles(states, words, nwords, sizes, lens[c0:c1], symtab[blk], F[blk], Cx[blk])
        if not ok.all():
            return None
        pieces += [out[i, :lens[c0 + i]] for i in range(c1 - c0)]
    return np.concatenate(pieces).tobytes()


def decode_segments(streams, stream_bytes, lengths):
    """The concatenated streams of the segment form back to the concatenated segments; None when any stream is malformed or names
    another length than the caller's."""
    streams = bytes(streams)
    if len(stream_bytes) != len(lengths) or sum(int(x) for x in stream_bytes) != len(streams):
        return None
    out, at = [], 0
    for sb, ln in zip(stream_bytes, lengths):
        part = decode(streams[at:at + int(sb)], want_n=int(ln))
        if part is None:
            return None
        out.append(part)
        at += int(sb)
    return b"".join(out)
