"""Built inputs for the inverse's stages and fallbacks (tests/test_inverse_paths.py on the GPU, tests/test_inverse_model.py on the
CPU): every input is an inverse INPUT B (any bytes are one), small enough for the CPU model (tests/inverse_model.py) to walk.

A case = one input, the (g, mark) cells it runs in, and the tags its home cells are there for.  A tag names a path; it is checked
twice: on the CPU against the model's prediction for a fresh context (so the GPU file's coverage list is a condition the inputs
meet by construction), and on the GPU against the engine's report.

  overflow        the node pool overflows: [RETRY_DENSE, DONE], the second attempt with every element a splitter
  virtual         virtual nodes, no overflow
  need_log        (moments cells only) the moments give up: [NEED_LOG, DONE], the second attempt with the index log
  unit_rank       a cycle without a splitter longer than one lane may follow: the unit-node route
  second_collect  more unreached elements than the first lists hold: laid out and collected again
  nu2             node cycles without a level-2 splitter
  moments:R       (moments cells only) what the moments make of the unreached elements (inverse_model.moments_route): R =
                  arithmetic (classes missing one or two elements name them), cycles (the cycles of the named elements bring
                  the rest), search (classes listed and chased element by element), need_log (they give up; the budget's form
                  of it needs more than 4 Mi elements in the listed classes: test_attempts_chain_of_the_default_path)

Thinning of family x g x mark.  The mark only changes how the elements no walk reached are found, and which elements those are
is a property of (input, g).  So an input runs all four marks at its HOME g's -- those where the family table says its path lies
-- and at every other g of the matrix two cells: moments (the default chain, with its own fallback) and one of log / sentinel /
bytemap, taken in turn over (input, g) so that every (g, mark) pair occurs in the file.  Inputs of more than 2 MiB run their home
cells only.  INV_AMBIGUOUS needs n = 2^32 and stays out, as does RETRY_DENSE by a refused unit block (it needs the device to be
out of memory)."""
import numpy as np

import oracle_lib as O

G_MATRIX = (0, 2, 4, 5, 6, 8, 12)
MARKS = ("moments", "log", "sentinel", "bytemap")
ROT_N = (1 << 18) + 1


def rotation(n, c, middle=False):
    """1^(n-c) 0^c: LF is i -> i + c mod n.  middle: the same two symbols between a run of a smaller and a run of a larger one
    (768 and 512 fixed points in front and behind: the rotation keeps its alignment to every g <= 8)."""
    B = np.concatenate([np.full(n - c, 1, np.uint8), np.zeros(c, np.uint8)])
    if middle:
        B = np.concatenate([np.zeros(768, np.uint8), B + np.uint8(7), np.full(512, 200, np.uint8)])
    return B


def short_factors_text(words, length, tail, seed):
    """`words` distinct Lyndon words of `length` bytes in decreasing order (each starts with its only smallest byte), then one long
    Lyndon factor: the transform has `words` LF cycles of `length` elements scattered among the long factor's rotations
    (tests/test_gpu_parity.py::_short_factors_text, the same construction)."""
    rng = np.random.default_rng(seed)
    ws = set()
    while len(ws) < words:
        c = int(rng.integers(60, 200))
        ws.add(bytes([c]) + rng.integers(c + 1, 256, length - 1, dtype=np.uint8).tobytes())
    body = b"".join(sorted(ws, reverse=True))
    return np.frombuffer(body + b"\0" + rng.integers(1, 256, tail, dtype=np.uint8).tobytes(), dtype=np.uint8)


def short_factors(words, length, tail, seed):
    return O.forward(short_factors_text(words, length, tail, seed))


def descending_runs(n, sigma, seed):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.integers(0, sigma, size=n, dtype=np.uint8))[::-1].copy()
    cut = int(rng.integers(1, n))
    return O.forward(np.concatenate([x[cut:], x[:cut]]) + np.uint8(40))


def noisy_period(n, seed):
    rng = np.random.default_rng(seed)
    period = rng.integers(0, 4, size=int(rng.integers(3, 200)), dtype=np.uint8)
    x = np.resize(period, n).copy()
    hits = rng.integers(0, n, size=n // 2000)
    x[hits] = rng.integers(0, 4, size=hits.size, dtype=np.uint8)
    return O.forward(x + np.uint8(97))


def lyndon_twice(length, seed):
    """(w w) for a Lyndon word w: two equal factors."""
    rng = np.random.default_rng(seed)
    w = np.concatenate([np.array([3], np.uint8), rng.integers(4, 9, length - 1, dtype=np.uint8)])
    return O.forward(np.concatenate([w, w]))


def many_cycles(d, L, m):
    """A rotation with gcd(n, c) = d: d cycles of L elements, the residue classes mod d, each with its smallest element at another
    offset of its node."""
    n, c = d * L, d * m
    assert np.gcd(L, m) == 1
    return rotation(n, c)


class Case:
    def __init__(self, name, build, homes, tags=(), others=G_MATRIX):
        self.name, self.build, self.homes, self.tags = name, build, tuple(homes), frozenset(tags)
        self.others = tuple(g for g in others if g not in self.homes)


def _small_inputs():
    """The members of tests/test_gpu_parity.py's SMALL list below 64 symbols: s = 1 .. 4 splitters at g = 4."""
    from test_gpu_parity import SMALL
    return [(k, x) for k, x in SMALL if 0 < x.size < 64]


def _cases():
    cs = []
    # rotations that fill the node pool with virtual nodes (n = 1 mod 2^g, c a multiple of 2^g)
    for c, g, tag in ((16 * 164, 4, "overflow"), (16000, 4, "virtual"), (64 * 41, 6, "virtual"), (256 * 11, 8, "virtual")):
        for mid in (False, True):
            cs.append(Case("rot%s-c%d-g%d" % ("mid" if mid else "", c, g), lambda c=c, mid=mid: rotation(ROT_N, c, mid), [g], [tag],
                           others=() if mid else G_MATRIX))
    # n = 2^k: half, or 15 of 16, of the elements in long cycles without a splitter
    cs.append(Case("rot2k-c2odd", lambda: rotation(1 << 18, 2 * 25001), [4], ["need_log", "unit_rank", "moments:need_log"]))
    cs.append(Case("rot2k-c32odd", lambda: rotation(1 << 18, 32 * 1001), [4], ["unit_rank", "nu2", "moments:search"]))
    cs.append(Case("rot2k-c2odd-17", lambda: rotation(1 << 17, 50002), [4, 8], ["unit_rank"], others=(4, 8)))
    # sorted bytes: LF is the identity, everything but the splitters is unreached: below, above and far above the first lists' room
    cs.append(Case("sorted-below", lambda: np.sort(O.generate("zipf", 1_115_000, 2)), [4], [], others=(4,)))
    cs.append(Case("sorted-above", lambda: np.sort(O.generate("zipf", 1_123_000, 2)), [4], ["second_collect"], others=(4, 5, 8)))
    cs.append(Case("sorted-far", lambda: np.sort(O.generate("zipf", 3 << 20, 2)), [4], ["second_collect"], others=(4,)))
    # short Lyndon factors in numbers: few -> the moments' arithmetic, more -> their cycles, many -> the chase, the budget, the log
    # (the route each is there for at g = 4, by the model's replay of the moments' rules: test_inverse_model.py checks the pins)
    routes = {(2, 1): "arithmetic", (2, 40): "arithmetic", (2, 600): "cycles", (2, 8000): "search",
              (3, 40): "arithmetic", (3, 600): "cycles", (3, 20000): "search",
              (9, 1): "arithmetic", (9, 40): "cycles", (9, 600): "cycles", (9, 20000): "search",
              (20, 40): "arithmetic", (20, 600): "cycles", (20, 20000): "search", (60, 600): "cycles", (60, 20000): "search"}
    for length, counts in ((2, (1, 40, 600, 8000)), (3, (1, 40, 600, 20000)), (9, (1, 40, 600, 20000)), (20, (1, 40, 600, 20000)),
                           (60, (1, 40, 600, 20000)), (300, (1, 40, 600, 4000))):
        for words in counts:
            big = words * length > 200000
            tags = (["nu2"] if (length == 300 and words >= 600) else []) + (["moments:" + routes[(length, words)]] if (length, words) in routes else [])
            cs.append(Case("short-l%d-w%d" % (length, words),
                           lambda words=words, length=length, big=big: short_factors(words, length, (1 << 18) if big else (1 << 20), 1000 + length + words),
                           [4], tags,
                           others=G_MATRIX if words in (40, 600) and length in (3, 20, 300) else (4,)))
    cs.append(Case("descending-runs", lambda: descending_runs(180001, 16, 5), [4]))
    cs.append(Case("noisy-period", lambda: noisy_period(150000, 6), [4]))
    cs.append(Case("lyndon-twice", lambda: lyndon_twice(70001, 7), [4]))
    # g >= 5, several threads to a node: cycles of 16 k + r elements, their smallest element anywhere in a node
    for r in (0, 1, 15):
        cs.append(Case("cycles-r%d" % r, lambda r=r: many_cycles(101, 4160 + r, 1009), [5, 6, 8, 12], [], others=(4, 5, 6, 8, 12)))
        cs.append(Case("short-l%d-w300" % (160 + r), lambda r=r: short_factors(300, 160 + r, 1 << 18, 50 + r), [5, 6], [],
                       others=(4, 5, 6, 8, 12)))
    for k, x in _small_inputs():
        cs.append(Case("small-" + k, lambda x=x: x, [4], [], others=(0, 2, 4, 5)))
    return cs


CASES = _cases()
WRAP_CASES = [c.name for c in CASES if c.name.startswith("cycles-r") or c.name.startswith("short-l16") or c.name.startswith("short-l17")]


def cells(case, index):
    """The (g, mark, home) cells of a case, by the thinning rule above."""
    out = [(g, m, True) for g in case.homes for m in MARKS]
    for j, g in enumerate(case.others):
        out.append((g, "moments", False))
        out.append((g, MARKS[1 + (index + j) % 3], False))
    return out


ALL_CELLS = [(c, g, m, home) for i, c in enumerate(CASES) for g, m, home in cells(c, i)]


def tag_holds(tag, chain, mark):
    """Does this chain of attempts (predicted, or reported and normalised by the test) show the path `tag` names?  None: the tag
    does not apply to this cell."""
    last = chain[-1]
    if tag == "overflow":
        return len(chain) == 2 and chain[0]["outcome"] == "RETRY_DENSE" and chain[0]["overflow"] and chain[1]["g"] == 0 and \
            chain[1]["mark"] == ("bytemap" if mark == "bytemap" else "sentinel") and last["outcome"] == "DONE"
    if tag == "virtual":
        return len(chain) == 1 and chain[0]["virtual"] > 0 and not chain[0]["overflow"]
    if tag == "need_log":
        if mark != "moments":
            return None
        return len(chain) == 2 and chain[0]["outcome"] == "NEED_LOG" and chain[1]["mark"] == "log" and chain[1]["g"] == chain[0]["g"]
    if tag == "unit_rank":
        return bool(last.get("unit_rank"))
    if tag == "second_collect":
        return bool(last.get("second_collect"))
    if tag == "nu2":
        return last.get("nu2", 0) > 0
    if tag.startswith("moments:"):
        if mark != "moments":
            return None
        return chain[0]["mark"] == "moments" and chain[0]["moments"]["route"] == tag[8:]
    raise KeyError(tag)


COVERAGE = ["finish:" + m for m in MARKS] + ["outcome:RETRY_DENSE", "outcome:NEED_LOG", "outcome:DONE", "virtual-without-overflow",
                                               "nu2", "second_collect", "unit_rank"] + ["g:%d" % g for g in G_MATRIX] + \
    ["moments:" + r for r in ("arithmetic", "cycles", "search", "need_log")]


def coverage_of(chain):
    """The items of COVERAGE a chain of attempts shows."""
    seen = set()
    for a in chain:
        if a.get("outcome"):
            seen.add("outcome:" + a["outcome"])
        seen.add("g:%d" % a["g"])
        if a.get("moments"):
            seen.add("moments:" + a["moments"]["route"])
        if a.get("outcome") == "DONE":
            seen.add("finish:" + a["mark"])
            for k in ("second_collect", "unit_rank"):
                if a.get(k):
                    seen.add(k)
            if a.get("nu2", 0) > 0:
                seen.add("nu2")
        if a.get("virtual", 0) > 0 and not a.get("overflow"):
            seen.add("virtual-without-overflow")
    return seen
