"""GPU suite (-m gpu): the lean last pass of round 0 (csrc/radix.hip, radix_scatter_lean_last_kernel): with 40-bit keys and few ties
expected, the fifth packed pass writes the carried byte and, instead of the sorted keys and the suffix array, the group flags of its
own output and the positions of the tied slots.

Every case compares the device's bytes with the oracle's exactly AND asserts header word 37 of the engine's report (0 not tried,
1 held, 2 gave up on a seam run, 3 on the tied count, 4 the direct form gave up behind it), so a silent fallback cannot make a case
pass.  The cells fix the key (BWTS_VARLEN=0 BWTS_KEY_SYMBOLS=5 over an 8-bit alphabet: 40 bits, five passes) and open the direct
form's gate (BWTS_DIRECT_MIN_LOG2=0).  The inputs are one Lyndon factor (a single smallest byte in front), so the key of position p
is its five bytes read cyclically, the last pass's input is the stable sort of the positions by the low four of them and its output
the stable sort by all five: layout() computes both, and every test asserts the property it is there for from that before it touches
the GPU.  A held case also runs with BWTS_RX_LEAN=0 and asks for the same report: tied count, form and rounds are what the flags of
group_flags_kernel give."""
import numpy as np
import pytest

import forward_cases as FC
import oracle_lib as O
import os

from test_direct_ties import DIRECT_GROUP, FELL_BACK_DEPTH, FELL_BACK_GROUP, LONG_PERIODS, fresh_context
from test_direct_ties import run as _run

pytestmark = pytest.mark.gpu

TILE = 8192               # csrc/radix.hip: elements of a scatter tile
SEAM = 64                 # ... elements the lean pass looks at on either side of a tile
REACH = 1024              # ... and how far it follows a run of equal low words that fills them, before it gives up
NOT_TRIED, HELD, GAVE_UP_SEAM, GAVE_UP_COUNT, GAVE_UP_DIRECT = 0, 1, 2, 3, 4
M = 5                     # symbols per key


def run(pkg, x, m, env=None, gate="0"):
    """test_direct_ties.run with the lean switch out of the way: a BWTS_RX_LEAN the process inherited reaches no case that does not
    set the switch itself."""
    saved = os.environ.pop("BWTS_RX_LEAN", None)
    try:
        return _run(pkg, x, m, env=env, gate=gate)
    finally:
        if saved is not None:
            os.environ["BWTS_RX_LEAN"] = saved


def base(n, seed):
    """Noise over 1 .. 254 behind a single 0: one Lyndon factor."""
    x = FC.noise(n, 254, seed, base=1)
    x[0] = 0
    return x


def layout(x):
    """K: the key of every position; lo, dig: its low four symbols and its first; rank: its place in the last pass's input; slot: its
    place in the output; tied: its key occurs more than once."""
    n = x.size
    assert O.lyndon_starts(x).tolist() == [0] and np.unique(x).size > 128, "one factor, 8-bit codes"
    p = np.arange(n)
    K = np.zeros(n, dtype=np.uint64)
    for j in range(M):
        K = (K << np.uint64(8)) | x[(p + j) % n].astype(np.uint64)
    lo = K & np.uint64(0xffffffff)
    rank, slot = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    rank[np.argsort(lo, kind="stable")] = p
    slot[np.argsort(K, kind="stable")] = p
    _, inv, cnt = np.unique(K, return_inverse=True, return_counts=True)
    return {"K": K, "lo": lo, "dig": (K >> np.uint64(32)).astype(np.int64), "rank": rank, "slot": slot, "tied": cnt[inv] > 1,
            "sizes": cnt[cnt > 1]}


def word_between(a, b, nbytes):
    """A value strictly between a and b whose `nbytes` bytes all lie in 1 .. 254 (it may go into an input without making a factor)."""
    for v in range(int(a) + (int(b) - int(a)) // 2, int(b)):
        w = [(v >> (8 * (nbytes - 1 - j))) & 255 for j in range(nbytes)]
        if all(1 <= c <= 254 for c in w):
            return w
    raise AssertionError("no room between %x and %x" % (a, b))


def check_held(pkg, x, L):
    """Lean on: held, the direct form settled everything, exact bytes; lean off: the same report."""
    tied = int(L["tied"].sum())
    assert 0 < tied <= x.size // 32 and L["sizes"].max() <= DIRECT_GROUP
    want = O.forward(x)
    got, t, reps = run(pkg, x, M)
    assert np.array_equal(got, want)
    rep = reps[-1]
    assert rep["lean_word"] == HELD and rep["keys"] == "split40", rep
    assert rep["tied0"] == tied and rep["form"] == "direct" and rep["rounds"] == 2 and rep["left"] == 0, rep
    got0, _, reps0 = run(pkg, x, M, env={"BWTS_RX_LEAN": "0"})
    assert np.array_equal(got0, want)
    assert reps0[-1]["lean_word"] == NOT_TRIED
    assert same_but_lean(rep) == same_but_lean(reps0[-1])


def same_but_lean(rep):
    return {k: v for k, v in rep.items() if k not in ("lean", "lean_word")}


def check_fallback(pkg, x, m, word):
    """Lean on: gave up with `word`, exact bytes, and words 0 .. 36 and the round records of the lean-off run."""
    want = O.forward(x)
    got, _, reps = run(pkg, x, m)
    assert np.array_equal(got, want)
    assert reps[-1]["lean_word"] == word and reps[-1]["keys"] == "split40", reps[-1]
    got0, _, reps0 = run(pkg, x, m, env={"BWTS_RX_LEAN": "0"})
    assert np.array_equal(got0, want)
    assert reps0[-1]["lean_word"] == NOT_TRIED
    assert same_but_lean(reps[-1]) == same_but_lean(reps0[-1])
    return reps[-1]


# ---- inside a tile ----------------------------------------------------------------------------------------------------------------
def inside_tile_input(n=9 * TILE + 4097, seed=51):
    """Pairs and groups of 3 .. 8 equal keys in noise, and one pair whose output slots are the last of a 64-slot word and the first
    of the next.  Returns (x, layout, the pair's positions)."""
    rng = np.random.default_rng(seed + 1000)               # (not the noise's own stream: its words would turn up in the noise)
    x0 = base(n, seed)
    sizes = [2] * 24 + [3, 4, 5, 6, 7, 8] * 2
    at = rng.permutation(np.arange(8, n // 16 - 8))[:sum(sizes)] * 16       # 16 apart: no two planted words touch
    for g in sizes:
        w = rng.integers(1, 255, size=M, dtype=np.uint8)
        for p in at[:g]:
            x0[p:p + M] = w
        at = at[g:]
    p1, p2 = 40, 72                                                          # (below 8 * 16: nothing else was planted here)
    # (the word's own bytes move a few neighbours' keys across it: the slot wanted is tried first, then the ones beside it)
    Ks = np.sort(layout(x0)["K"])
    for s in sorted(range(64 * 499, 64 * 503), key=lambda s: abs(s - (64 * 500 + 63))):
        x = x0.copy()
        x[p1:p1 + M] = x[p2:p2 + M] = word_between(Ks[s - 1], Ks[s], M)
        L = layout(x)
        if L["slot"][p1] % 64 == 63:
            return x, L, (p1, p2)
    raise AssertionError("the pair did not land on a word boundary")


def test_inside_a_tile(pkg):
    x, L, (p1, p2) = inside_tile_input()
    n = x.size
    assert n % TILE == 4097 and n % 64 != 0
    assert sorted(np.bincount(L["sizes"])[2:].tolist()) == sorted(np.bincount([2] * 25 + [3, 4, 5, 6, 7, 8] * 2)[2:].tolist()), L["sizes"]
    assert L["K"][p1] == L["K"][p2] and L["slot"][p1] % 64 == 63 and L["slot"][p2] == L["slot"][p1] + 1
    check_held(pkg, x, L)


# ---- seams ------------------------------------------------------------------------------------------------------------------------
def seam_input(n, seed, t, digits, before):
    """A cluster of len(digits) positions that share their low four symbols, their first symbols `digits` in position order, placed
    so that `before` of them come before place t * TILE of the last pass's input and the rest from there on."""
    x0 = base(n, seed)
    x0[30000:30000 + M] = x0[50000:50000 + M]              # one pair far from the seam: the direct form always has something to settle
    pos = 1000 + 16 * np.arange(len(digits))
    # (the cluster's own bytes move a few neighbours across it: the place wanted is tried first, then the ones beside it)
    los = np.sort(layout(x0)["lo"])
    for R in sorted(range(t * TILE - before - 32, t * TILE - before + 33), key=lambda R: abs(R - (t * TILE - before))):
        V = word_between(los[R - 1], los[R], 4)
        x = x0.copy()
        for p, d in zip(pos, digits):
            x[p:p + M] = [d] + V
        L = layout(x)
        if L["rank"][pos[0]] == t * TILE - before:
            return x, L, pos
    raise AssertionError("the cluster did not land on the seam")


SEAMS = [
    # name, tile seam, first symbols of the cluster in position order, members before the seam, members expected tied
    ("pair-split", 3, [3, 9, 9, 5], 2, [1, 2]),
    ("three-middle-last-before", 5, [7, 7, 11, 7, 12], 2, [0, 1, 3]),
    ("three-middle-first-after", 2, [7, 13, 7, 7], 2, [0, 2, 3]),
    ("no-tie", 4, [1, 2, 3, 4, 5, 6], 3, []),
    # noise never holds 255: the digit occurs on one side of the seam only, and nowhere else in that tile
    ("digit-absent-before", 6, [4, 6, 255, 255], 2, [2, 3]),
    ("digit-absent-after", 9, [255, 255, 4, 6], 2, [0, 1]),             # (the tile behind this seam is the partial last one)
]


@pytest.mark.parametrize("name,t,digits,before,tied", SEAMS, ids=[c[0] for c in SEAMS])
def test_seams(pkg, name, t, digits, before, tied):
    n = 9 * TILE + 100
    x, L, pos = seam_input(n, 60 + t, t, digits, before)
    c = len(digits)
    assert c < SEAM and np.array_equal(np.flatnonzero(L["lo"] == L["lo"][pos[0]]), pos), "the cluster and nobody else"
    assert np.array_equal(L["rank"][pos], t * TILE - before + np.arange(c)) and 0 < before < c, "it straddles the seam"
    assert np.flatnonzero(L["tied"][pos]).tolist() == tied
    if 255 in digits:
        side = slice((t - 1) * TILE, t * TILE) if name == "digit-absent-before" else slice(t * TILE, (t + 1) * TILE)
        by_rank = np.argsort(L["rank"])
        assert not (L["dig"][by_rank[side]] == 255).any() and (L["dig"] == 255).sum() == 2
    assert L["tied"].sum() == len(tied) + 2 and L["tied"][[30000, 50000]].all()
    check_held(pkg, x, L)


# ---- runs longer than the first look across a seam -----------------------------------------------------------------------------
def cluster_word(a, b, second_below):
    """A low word strictly between a and b, bytes in 1 .. 254, its last two above its first and its second below it or not; or None."""
    for hi in range(int(a) >> 16, (int(b) >> 16) + 1):
        w0, w1 = hi >> 8, hi & 255
        if not (1 <= w0 <= 252 and 1 <= w1 <= 254 and (w1 < w0) == second_below):
            continue
        for w2 in range(w0 + 1, 255):
            v = (hi << 16) | (w2 << 8) | 254
            if int(a) < v < int(b):
                return [w0, w1, w2, 254]
    return None


def long_seam_input(n, seed, t, digits, before):
    """seam_input for clusters of hundreds.  Every member moves the positions next to it (their low words hold the cluster's bytes)
    to one side of the cluster or the other, by how the cluster's bytes compare among themselves.  So the low word is taken with its
    last two bytes above its first and its second on one chosen side of the first: then that side is the same for every candidate,
    the cluster lands a nearly constant distance from where its low word was aimed, and stepping by the miss finds the place."""
    x0 = base(n, seed)
    x0[30000:30000 + M] = x0[50000:50000 + M]
    pos = 1000 + 16 * np.arange(len(digits))
    assert pos[-1] + M < 30000
    los = np.sort(layout(x0)["lo"])
    want = t * TILE - before
    for second_below in (True, False):
        R = want
        for _ in range(24):
            V = None
            for R in range(R, min(R + 600, n - 1)):               # the next place whose gap holds such a word
                V = cluster_word(los[R - 1], los[R], second_below)
                if V is not None:
                    break
            if V is None:
                break
            x = x0.copy()
            for i, (p, d) in enumerate(zip(pos, digits)):
                x[p:p + M + 1] = [d] + V + [1 + 7 * i % 254]       # (the byte behind: the keys one place on tie in small groups too)
            L = layout(x)
            got = int(L["rank"][pos[0]])
            if got == want:
                return x, L, pos
            R = max(R + want - got, 1)
    raise AssertionError("the cluster did not land on the seam")


def check_cluster(L, pos, t, before):
    c = pos.size
    assert np.array_equal(np.flatnonzero(L["lo"] == L["lo"][pos[0]]), pos), "the cluster and nobody else"
    assert np.array_equal(L["rank"][pos], t * TILE - before + np.arange(c)) and 0 < before < c, "it straddles the seam"


def test_long_run_before_the_seam(pkg):
    """160 positions with one low word, 150 of them before a seam: the tile behind the seam follows the run through three windows.
    One of its members has its only partner 130 places before the seam (the third window); the digits of its other members occur
    nowhere in the run before the seam."""
    t, before = 3, 150
    digits = list(range(1, 161))
    digits[153] = digits[20]
    x, L, pos = long_seam_input(9 * TILE + 100, 95, t, digits, before)
    check_cluster(L, pos, t, before)
    assert SEAM < before < REACH and before - 20 > 2 * SEAM
    assert np.flatnonzero(L["tied"][pos]).tolist() == [20, 153]
    check_held(pkg, x, L)


def test_long_run_behind_the_seam_to_the_array_end(pkg):
    """155 positions with the largest low word of all, 150 of them behind the last seam: they are the whole partial last tile, and the
    tile before it follows the run through three windows, the last of which the array's end cuts short.  A member before the seam has
    its only partner 100 places behind it (the second window)."""
    c, after = 155, 150
    n = 9 * TILE + after
    x = base(n, 96)
    pos = 1000 + 16 * np.arange(c)
    digits = list(range(1, c + 1))
    digits[2] = digits[5 + 100]
    for p, d in zip(pos, digits):
        x[p:p + M] = [d, 255, 255, 255, 255]
    L = layout(x)
    check_cluster(L, pos, 9, c - after)
    assert L["rank"][pos[-1]] == n - 1 and SEAM < after < REACH and after % SEAM != 0
    assert np.flatnonzero(L["tied"][pos]).tolist() == [2, 105]
    check_held(pkg, x, L)


@pytest.mark.parametrize("before,word", [(REACH - 1, HELD), (REACH, GAVE_UP_SEAM)])
def test_reach(pkg, before, word):
    """A run that ends one short of the reach before a seam is followed to its end and decided (every one of its digits occurs four
    times and more: all its members are tied, in groups the direct form takes); one of exactly the reach is given up."""
    t = 5
    digits = [1 + i % 254 for i in range(before + 6)]
    x, L, pos = long_seam_input(9 * TILE + 100, 97, t, digits, before)
    check_cluster(L, pos, t, before)
    assert L["tied"][pos].all() and L["sizes"].max() <= DIRECT_GROUP and int(L["tied"].sum()) <= x.size // 32
    if word == HELD:
        check_held(pkg, x, L)
    else:
        check_fallback(pkg, x, M, word)


# ---- the array's ends -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65536, 65537])
def test_edges(pkg, n):
    """The two smallest keys equal (slots 0 and 1) and the two largest (slots n - 2 and n - 1)."""
    x = FC.noise(n, 253, 71, base=2)
    x[:6], x[6] = 0, 1                                  # 0^6 1 ...: one factor; positions 0 and 1 read 0 0 0 0 0
    x[3000:3000 + M] = x[9000:9000 + M] = 255
    L = layout(x)
    assert L["slot"][[0, 1]].tolist() == [0, 1] and L["tied"][[0, 1]].all()
    assert L["slot"][[3000, 9000]].tolist() == [n - 2, n - 1] and L["tied"][[3000, 9000]].all()
    check_held(pkg, x, L)


# ---- giving up --------------------------------------------------------------------------------------------------------------------
def test_seam_run_too_long(pkg):
    """8192 + 128 positions with the same low four symbols: their run covers some tile seam with at least 64 of them on either side,
    and reaches further from some seam than the pass follows it."""
    n, c = 1 << 20, TILE + 2 * SEAM
    x = base(n, 81)
    pos = 64 + 8 * np.arange(c)
    for i, p in enumerate(pos):
        x[p:p + M] = [1 + i % 254, 17, 34, 51, 68]
    L = layout(x)
    r = np.sort(L["rank"][L["lo"] == L["lo"][pos[0]]])
    assert r.size >= c and np.array_equal(r, r[0] + np.arange(r.size)), "one run"
    seams = [b for b in range(TILE, n, TILE) if b - r[0] >= SEAM and r[-1] + 1 - b >= SEAM]
    assert seams and int(L["tied"].sum()) <= n // 32
    assert [b for b in range(TILE, n, TILE) if r[0] < b <= r[-1] and max(b - r[0], r[-1] + 1 - b) >= REACH]
    check_fallback(pkg, x, M, GAVE_UP_SEAM)


def test_too_many_ties(pkg):
    """2600 pairs in 2^17 positions of noise: more than n / 32 tied, where the byte histogram (all the key model sees) expects a handful."""
    n = 1 << 17
    x = base(n, 91)
    for i in range(2600):
        x[48 * i + 24:48 * i + 24 + M] = x[48 * i + 48:48 * i + 48 + M]
    L = layout(x)
    assert int(L["tied"].sum()) > n // 32
    rep = check_fallback(pkg, x, M, GAVE_UP_COUNT)
    assert rep["form"] in ("chunks", "tiles") and rep["tied0"] == int(L["tied"].sum()), rep


def key_symbols_for_five_passes(x):
    bits = max(int(np.unique(x).size) - 1, 1).bit_length()
    assert 33 <= (40 // bits) * bits <= 40
    return 40 // bits


DIRECT_GIVES_UP = [("group-above-the-cap", lambda: FC.pasted(1 << 20, 4, 5, [(40, 200)]), FELL_BACK_GROUP)] + \
                  [(c[0], c[1], FELL_BACK_DEPTH) for c in LONG_PERIODS]


@pytest.mark.parametrize("name,build,direct", DIRECT_GIVES_UP, ids=[c[0] for c in DIRECT_GIVES_UP])
def test_direct_form_gives_up_behind_it(pkg, name, build, direct):
    """The inputs on which tests/test_direct_ties.py sees the direct form give up (a group above its cap; pairs equal beyond its
    depth), with as many symbols per key as make five passes: the lean pass held, the direct form gave the list back, and the classic
    last pass and the sparse rounds ran as without it."""
    x = build()
    rep = check_fallback(pkg, x, key_symbols_for_five_passes(x), GAVE_UP_DIRECT)
    assert rep["direct_word"] == direct and rep["form"] == "sparse" and 0 < rep["tied0"] <= x.size // 32, rep


# ---- not taken --------------------------------------------------------------------------------------------------------------------
NOT_TAKEN = [
    ("gather", M, {"BWTS_EMIT": "gather"}),
    ("general-lyndon-suffix-sort", M, {"BWTS_LYNDON": "general"}),
    ("32-bit-keys", 4, {}),
    ("switched-off", M, {"BWTS_RX_LEAN": "0"}),
]


@pytest.mark.parametrize("name,m,env", NOT_TAKEN, ids=[c[0] for c in NOT_TAKEN])
def test_not_taken(pkg, name, m, env):
    x, _, _ = inside_tile_input()
    got, _, reps = run(pkg, x, m, env=env)
    assert np.array_equal(got, O.forward(x))
    assert reps[0]["lean_word"] == NOT_TRIED and reps[0]["tied0"] > 0, reps[0]
    if name == "general-lyndon-suffix-sort":
        assert len(reps) == 2 and not reps[0]["cyclic"] and reps[1]["cyclic"]


def test_not_taken_two_segments(pkg):
    a, _, _ = inside_tile_input()
    b, _, _ = inside_tile_input(n=9 * TILE + 5, seed=52)
    x = np.concatenate([a, b])
    with fresh_context(pkg, {"BWTS_VARLEN": "0", "BWTS_KEY_SYMBOLS": str(M), "BWTS_DIRECT_MIN_LOG2": "0"}) as ctx:
        got = ctx.forward_segments(x, [a.size, b.size])
        reps = ctx.debug_forward_report()
    assert np.array_equal(got, np.concatenate([O.forward(a), O.forward(b)]))
    assert reps[-1]["cyclic"] and reps[-1]["tied0"] > 0 and reps[-1]["lean_word"] == NOT_TRIED, reps[-1]


def test_taken_after_a_segmented_call(pkg):
    """The table a segmented call leaves with the context means nothing to the plain call behind it."""
    a, La, _ = inside_tile_input()
    b, _, _ = inside_tile_input(n=9 * TILE + 5, seed=52)
    saved = os.environ.pop("BWTS_RX_LEAN", None)
    try:
        with fresh_context(pkg, {"BWTS_VARLEN": "0", "BWTS_KEY_SYMBOLS": str(M), "BWTS_DIRECT_MIN_LOG2": "0"}) as ctx:
            ctx.forward_segments(np.concatenate([a, b]), [a.size, b.size])
            assert ctx.debug_forward_report()[-1]["lean_word"] == NOT_TRIED
            got = ctx.forward(a)
            rep = ctx.debug_forward_report()[-1]
    finally:
        if saved is not None:
            os.environ["BWTS_RX_LEAN"] = saved
    assert np.array_equal(got, O.forward(a))
    assert rep["lean_word"] == HELD and rep["form"] == "direct" and rep["tied0"] == int(La["tied"].sum()), rep


def test_not_taken_below_the_default_gate(pkg):
    """No knob: below 2^24 positions the direct form is not the default, and the lean pass is nothing without it."""
    x = FC.noise((1 << 24) - 1, 4, 21)
    got, _, reps = run(pkg, x, None, gate=None)
    assert np.array_equal(got, O.forward(x))
    assert reps[-1]["lean_word"] == NOT_TRIED and reps[-1]["direct_word"] == 0 and reps[-1]["tied0"] > 0, reps[-1]


def test_default(pkg):
    """No knob, 2^24 positions of the benchmark's own source: the heuristics pick a 40-bit key and expect few ties; held."""
    x = O.generate("zipf", 1 << 24, 7)
    got, _, reps = run(pkg, x, None, gate=None)
    assert np.array_equal(got, O.forward(x))
    rep = reps[-1]
    assert rep["lean_word"] == HELD and rep["keys"] == "split40" and rep["form"] == "direct" and rep["rounds"] == 2, rep
    assert 0 < rep["tied0"] <= x.size // 32 and rep["left"] == 0, rep
