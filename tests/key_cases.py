"""Inputs and histograms for the round-0 key tests (tests/test_key_plan.py on the CPU, tests/test_round0_keys_gpu.py on the GPU).

Histogram families: counts in a fixed shape over `sigma` byte values spread across 0..255, every present count at least 1, summing to
n exactly.  Variable-key inputs: texts for which the layout rules pick variable-length keys by themselves (no knob), small enough for
the model (tests/key_model.py) to key every position."""
import numpy as np

import oracle_lib as O
import realtext

FAMILIES = ("uniform", "geometric", "fibonacci", "dominant_first", "dominant_middle")
N_VAR = (1 << 17) + 5


def family_hist(family, sigma, n, ratio=0.5):
    """256 counts: `sigma` present byte values, shaped by the family, summing to n (n >= sigma)."""
    assert 1 <= sigma <= 256 and n >= sigma
    if family == "uniform":
        w = [1] * sigma
    elif family == "geometric":
        w = [ratio ** i for i in range(sigma)]
    elif family == "fibonacci":
        w, a, b = [], 1, 1
        for _ in range(sigma):
            w.append(a)
            a, b = b, a + b
    elif family == "dominant_first":
        w = [1] + [0] * (sigma - 1)
    elif family == "dominant_middle":
        w = [0] * sigma
        w[sigma // 2] = 1
    else:
        raise KeyError(family)
    return shaped_hist(w, n)


def shaped_hist(w, n):
    """256 counts in proportion to the weights w (len(w) present byte values spread over 0..255), each at least 1, summing to n."""
    sigma = len(w)
    W = sum(w)
    spare = n - sigma
    counts = [1 + min(spare, int(spare * (wi / W))) for wi in w]
    top = max(range(sigma), key=lambda i: w[i])
    i = 0
    while sum(counts) > n:                          # (rounding may overshoot by a few)
        if counts[i % sigma] > 1:
            counts[i % sigma] -= 1
        i += 1
    counts[top] += n - sum(counts)
    hist = np.zeros(256, dtype=np.uint64)
    for i, c in enumerate(counts):
        hist[i * 256 // sigma] = c
    assert int(hist.sum()) == n and int((hist > 0).sum()) == sigma
    return hist


def byte_hist(x):
    return np.bincount(np.asarray(x, dtype=np.uint8), minlength=256).astype(np.uint64)


def geometric_text(n, symbols, ratio, seed, base=97):
    """n draws from a geometric distribution over `symbols` byte values from `base` on: value base + i with probability ~ ratio^i."""
    rng = np.random.default_rng(seed)
    p = ratio ** np.arange(symbols, dtype=np.float64)
    return (rng.choice(symbols, size=n, p=p / p.sum()) + base).astype(np.uint8)


def geo16(n=N_VAR, seed=16):
    return geometric_text(n, 16, 0.5, seed)


def geo40(n=N_VAR, seed=41):
    return geometric_text(n, 40, 0.8, seed, base=48)


def geo8(n, seed=8):
    return geometric_text(n, 8, 0.5, seed)


def text(n=N_VAR, seed=7):
    return O.generate("text", n, seed)


def real(n=1 << 17):
    return np.frombuffer(realtext.seed_text()[:n], dtype=np.uint8).copy()


# the inputs of the exact variable-length cells: name -> builder
VARLEN_INPUTS = {"geo16": geo16, "geo40": geo40, "text": text, "real": real}


def rarest_and_commonest(x):
    """(the present byte value seen least often, the one seen most often): in a geometric text the longest and the shortest code word."""
    h = np.bincount(x, minlength=256)
    present = np.flatnonzero(h)
    return int(present[np.argmin(h[present])]), int(present[np.argmax(h[present])])


def word_seams(k, seed=3):
    """Geometric text of (1 << 16) + 2048 + k bytes for the bit stream's word seams: runs of the commonest symbol (a 1-bit word) of
    30 .. 34 and 62 .. 66 symbols, so that code words and key windows start at every bit offset of a stream word, and the rarest
    symbol (the longest word) right before the key builder's tile ends (positions 2047, 2048, 8190 .. 8192) and, four times, inside
    the text's last 64 positions, where the stream is zero-filled past the end."""
    n = (1 << 16) + 2048 + k
    x = geo16(n, seed)
    rare, common = rarest_and_commonest(x)
    at = 300
    for length in (30, 31, 32, 33, 34, 62, 63, 64, 65, 66):
        for _ in range(3):
            x[at:at + length] = common
            x[at + length] = common + 1
            at += length + 37                      # (odd gaps: the runs start at varying offsets)
    for p in (2047, 2048, 8190, 8191, 8192, n - 61, n - 33, n - 2, n - 1):
        x[p] = rare
    return x


def descending_lyndon_words_geometric(n, seed, lmin=2, lmax=70):
    """Words of lmin .. lmax bytes whose first byte (1) is smaller than all their others, in non-increasing order: the input's Lyndon
    factors are exactly these words.  Bodies are draws from the geometric distribution over 16 byte values."""
    rng = np.random.default_rng(seed)
    words, total = [], 0
    while total < n:
        L = int(rng.integers(lmin, (lmax if rng.integers(2) else 12) + 1))      # every second word is short: > 1000 factors in 24 KiB
        words.append(bytes([1]) + geometric_text(L - 1, 16, 0.5, int(rng.integers(1 << 30))).tobytes())
        total += L
    words.sort(reverse=True)
    return np.frombuffer(b"".join(words)[:n], dtype=np.uint8).copy()


def planted_runs(spec, sym, seed=16, n=N_VAR):
    """geo16 with runs of the byte value `sym` planted.  spec: [(run length, [the byte behind the run, one per copy])]: every copy of
    a run is followed by its own byte (the first symbol a key of the run alone does not cover) and stands behind a byte that varies
    too.  Returns (x, {run length: [where its copies start]})."""
    x = geo16(n, seed)
    _, common = rarest_and_commonest(x)
    at, where = 5000, {}
    for length, followers in spec:
        for i, f in enumerate(followers):
            where.setdefault(length, []).append(at)
            x[at - 1] = common + 2 + (i % 3)
            x[at:at + length] = sym
            x[at + length] = f
            x[at + length + 1] = common + (i // 8) % 8
            at += 997
    return x, where
