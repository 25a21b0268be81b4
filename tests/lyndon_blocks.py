"""Inputs whose Lyndon factors come from runs of the smallest byte (zeros in tar files, disk images, executables): so many positions tie
with the running minimum of the round-0 keys that the candidate search cannot settle them, and the n > 2^32 forward takes the suffix
route (wide_path.h).  Two shapes:

  lyndon_blocks  blocks of 0^L followed by a body of bytes 1..255, L never decreasing, blocks of equal L in descending byte order.  Every
                 block is a Lyndon word and the sequence does not increase, so the factors are exactly the blocks (Chen-Fox-Lyndon).
  tar_like       random non-zero bytes broken by zero runs of random length."""
import numpy as np


def lyndon_blocks(nblocks, L, body_lo, body_hi, seed):
    """nblocks blocks, block i = 0^L[i] + body; L non-decreasing.  Among blocks of equal L the bodies open with a 3-byte counter (base
    255, digits 1..255) that falls from block to block, so the descending order needs no sort at any size.  Returns (x, starts)."""
    rng = np.random.default_rng(seed)
    L = np.asarray(L, dtype=np.int64)
    assert L.size == nblocks and np.all(np.diff(L) >= 0) and L.min() >= 1
    blen = rng.integers(body_lo, body_hi + 1, size=nblocks, dtype=np.int64)
    assert body_lo >= 3
    size = L + blen
    starts = np.zeros(nblocks, dtype=np.int64)
    np.cumsum(size[:-1], out=starts[1:])
    n = int(starts[-1] + size[-1])
    x = np.empty(n, dtype=np.uint8)
    step = 1 << 28
    for o in range(0, n, step):
        x[o:o + step] = rng.integers(1, 256, size=min(step, n - o), dtype=np.uint8)
    for s, l in zip(starts.tolist(), L.tolist()):
        x[s:s + l] = 0
    # rank of the block inside its run of equal L, counted from the run's end: the counter falls along the run
    last = np.searchsorted(L, L, side="right")
    c = (last - 1 - np.arange(nblocks)).astype(np.int64)
    assert c.max() < 255 ** 3
    b0 = starts + L
    x[b0] = (c // (255 * 255) + 1).astype(np.uint8)
    x[b0 + 1] = ((c // 255) % 255 + 1).astype(np.uint8)
    x[b0 + 2] = (c % 255 + 1).astype(np.uint8)
    return x, starts


def small_lyndon_blocks(seed=1):
    """3000 blocks, L from 17 rising by one every 30 blocks (to 116), bodies of 20..200 bytes: about 0.5 MB, 150 000 positions
    followed by 17 or more zeros."""
    nb = 3000
    return lyndon_blocks(nb, 17 + np.arange(nb) // 30, 20, 200, seed)


def big_lyndon_blocks(n_target, seed=7):
    """Blocks of L = 65 + i // 2^16 zeros and 200..2000 body bytes until n_target bytes are reached: about 3.8 M blocks at
    n = 2^32 + 2^28, L up to about 123, 3.6 * 10^8 zeros (far below one 12-bit key prefix's bucket)."""
    avg = 65 + 1100 + 30
    nb = int(n_target // avg) + 1
    return lyndon_blocks(nb, 65 + np.arange(nb) // (1 << 16), 200, 2000, seed)


def tar_like(n_chunks, seed):
    """Random non-zero chunks of 50..2000 bytes, each followed by a zero run: a third of them 1..63 bytes, the rest 64..700."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(n_chunks):
        parts.append(rng.integers(1, 256, size=int(rng.integers(50, 2001)), dtype=np.uint8))
        z = int(rng.integers(1, 64)) if rng.random() < 1 / 3 else int(rng.integers(64, 701))
        parts.append(np.zeros(z, dtype=np.uint8))
    return np.concatenate(parts)


def positions_before_zero_runs(x, run):
    """Positions followed by at least `run` zeros (themselves included)."""
    z = np.concatenate([(x == 0).astype(np.int64), np.zeros(1, np.int64)])
    # length of the zero run starting at each position
    idx = np.flatnonzero(z == 0)                       # positions of non-zeros (and the sentinel)
    nxt = idx[np.searchsorted(idx, np.arange(x.size), side="left")]
    return int(np.count_nonzero(nxt - np.arange(x.size) >= run))
