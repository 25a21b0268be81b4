"""Real text for the repeat-rich regime (the reference's own workload is enwik8, Makefile:35-38, which is not part of this project).

The material is the project's own documentation and source text -- the .md, .py, .c, .h, .hip files and Makefiles of the tree, in
sorted path order, concatenated (1.0 MB, 141 distinct bytes) -- stored once as tests/golden/realtext_seed.xz, so the corpus is
the same wherever the repository is checked out.  A corpus is a stream of "files": pieces of that text of 256 B .. 64 KiB (log-uniform
length, uniform offset), each with one byte in about 2 KiB replaced by a byte from elsewhere in the text -- the long but imperfect
repeats that a directory of related sources and documents has.  Every choice comes from a seeded splitmix64 stream, so the bytes depend
on nothing but the seed file.  Test infrastructure: the gpu tests hold the corpus to the sha-256 on file (tests/golden/realtext.json and
realtext_1GiB.json, made by tests/golden/make_golden_realtext.py and make_golden_realtext_big.py)."""
import lzma
import os

SEED_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realtext_seed.xz")
_M64 = (1 << 64) - 1
_seed_text = None


def seed_text():
    global _seed_text
    if _seed_text is None:
        with open(SEED_FILE, "rb") as f:
            _seed_text = lzma.decompress(f.read())
    return _seed_text


def _splitmix64(state):
    while True:
        state = (state + 0x9E3779B97F4A7C15) & _M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        yield z ^ (z >> 31)


def _assemble(limit, stream_seed):
    text = seed_text()
    s = len(text)
    rnd = _splitmix64(stream_seed)
    out = bytearray(limit)
    at = 0
    while at < limit:
        # length 2^(8 + 8 u), u uniform in [0, 1) on 16 bits: 256 B .. 64 KiB
        length = min(int(2.0 ** (8.0 + 8.0 * ((next(rnd) >> 48) / 65536.0))), limit - at)
        src = next(rnd) % (s - length + 1)
        out[at:at + length] = text[src:src + length]
        for _ in range(length // 2048 + 1):
            r = next(rnd)
            out[at + (r & 0xFFFFFFFF) % length] = text[(r >> 32) % s]
        at += length
    return bytes(out)


def corpus(limit):
    """`limit` bytes of the corpus (the gpu suite's real-text input is 2^26 of them: tests/golden/realtext.json)."""
    return _assemble(limit, 1)


def corpus_big(limit):
    """The same kind of material from a stream of its own, up to `limit` bytes: the >= 1 GiB real-text input
    (tests/golden/realtext_1GiB.json), where every piece of the text recurs about a thousand times."""
    return _assemble(limit, 2)
