"""The forward's sort rounds from their definition, in numpy: no GPU, no engine code.

The bijective BWT sorts every position p by the infinite word that starts at p and runs round and round its own Lyndon factor
(the suffix form: by the suffix at p, which ends at n and is followed by something smaller than every symbol).  The engine sorts
by the first m symbols (round 0), then refines: a round at step h reads the ranks at depth h of p and of its successors at distance
h (sparse form: one successor, depth 2h) or h, 2h, 3h (chunks and tiles: depth 4h).  All gathers of a round read one version of the
ranks, and the moves are applied after them, so the partition after round r is EXACTLY the classes of positions by their first
m * 2^r (m * 4^r) symbols -- never finer, never coarser.  Model.classes(d) computes those classes by composing: depth a + b from depth a
at p and depth b at the a-th successor of p.  Class ids are order-preserving (a smaller id is a smaller word), so the last partition
also gives the transform itself (Model.transform).

predict() replays the host rules that pick a path from those counts (which form, the probe's rules, the big list's split and drain,
rounds per host trip, the compaction trigger); the thresholds below are the ones DESIGN.md states for the engine."""
import numpy as np

import oracle_lib as O

CH_CAP = 256              # groups of up to this many members go to chunks at once (and are "small" for the tile form)
CH_GROUP_MAX = 2048       # a group of up to this many members leaves the big list for a WIDE chunk
CH_MIN_LIST = 65536       # shorter lists keep the tile form
CH_FS = 256               # at most this many factors: their starts sit in LDS
SEG_CAP = 8               # sparse form: larger groups go through the radix sort
SEG_MIN_LIST = 4096       # sparse form: lists of at most this are sorted whole, no probe
RANK_EARLY_N = 1 << 22
FLAGS_OUTSIDE_N = 4096
MAX_ROUNDS = 80
CHUNK_TARGET = 16384      # chunks a cut aims at (the test switch BWTS_CHUNK_TARGET lowers it)


class Model:
    def __init__(self, x, cyclic=True):
        self.x = np.ascontiguousarray(x, dtype=np.uint8)
        self.n = n = self.x.size
        self.cyclic = cyclic
        if cyclic:
            self.starts = O.lyndon_starts(self.x).astype(np.int64)
            lens = np.diff(np.append(self.starts, n))
            self.fs = np.repeat(self.starts, lens)
            self.fl = np.repeat(lens, lens)
            self.k = self.starts.size
        else:
            self.starts, self.k = None, 0
        _, sym = np.unique(self.x, return_inverse=True)
        self._cls = {1: sym.astype(np.int64) + (0 if cyclic else 1)}      # (suffix form: id 0 is "past the end")
        self._stats = {}

    def succ(self, a):
        """The a-th successor of every position: within its factor, wrapping at the factor's end.  Suffix form: p + a, n = past the end."""
        p = np.arange(self.n, dtype=np.int64)
        if self.cyclic:
            return self.fs + (p - self.fs + np.mod(int(a), self.fl)) % self.fl
        return np.minimum(p + min(int(a), self.n), self.n)

    def compose(self, ca, a, cb):
        """Classes at depth a + b from those at depth a (ca) and at depth b (cb): the pair (ca[p], cb[a-th successor of p])."""
        s = self.succ(a)
        if self.cyclic:
            cbs = cb[s]
        else:
            cbs = np.append(cb, 0)[s]
        key = ca * (int(cb.max()) + 1) + cbs
        _, inv = np.unique(key, return_inverse=True)
        return inv.astype(np.int64) + (0 if self.cyclic else 1)

    def classes(self, d):
        d = int(d)
        if d not in self._cls:
            a = d - d // 2
            self._cls[d] = self.compose(self.classes(a), a, self.classes(d - a))
        return self._cls[d]

    def sizes(self, d):
        """The size of every position's class at depth d."""
        c = self.classes(d)
        return np.bincount(c)[c]

    def stats(self, d):
        d = int(d)
        if d not in self._stats:
            c = self.classes(d)
            cnt = np.bincount(c)
            sz = cnt[c]
            self._stats[d] = {
                "depth": d, "classes": int(np.count_nonzero(cnt)), "tied": int((sz > 1).sum()),
                "le_cap": int(((sz > 1) & (sz <= CH_CAP)).sum()), "mid": int(((sz > CH_CAP) & (sz <= CH_GROUP_MAX)).sum()),
                "huge": int((sz > CH_GROUP_MAX).sum()), "huge_groups": int((cnt > CH_GROUP_MAX).sum()), "gt_seg": int((sz > SEG_CAP).sum()),
            }
        return self._stats[d]

    def walk(self, m, step):
        """Round 0 at depth m, then rounds that multiply the depth by `step`: [stats per depth], the stop reason.  The cyclic form stops
        when the list is empty or a round splits no group (then nothing ever will: the classes are those of the infinite words);
        the suffix form stops when the list is empty, which it reaches at depth n at the latest."""
        out = [self.stats(m)]
        if out[0]["tied"] == 0:
            return out, "none"
        d = int(m)
        while True:
            d *= step
            out.append(self.stats(d))
            if out[-1]["tied"] == 0:
                return out, "empty"
            if self.cyclic and out[-1]["classes"] == out[-2]["classes"]:
                return out, "stable"
            assert len(out) <= MAX_ROUNDS and (self.cyclic or d < 4 * self.n), "the suffix form must end"

    def final_tied(self, m=1):
        """Elements in groups of equal infinite words (cyclic form)."""
        return self.walk(m, 2)[0][-1]["tied"]

    def transform(self):
        """The bijective BWT from the classes alone: positions in class order, each giving the byte in front of it within its factor."""
        st, _ = self.walk(1, 2)
        c = self.classes(st[-1]["depth"])
        order = np.argsort(c, kind="stable")
        prev = self.fs[order] + (order - self.fs[order] - 1) % self.fl[order]
        return self.x[prev]


def key_form(key_bits, n, carry, pack=True):
    """How round 0 keeps its keys: the packed passes take keys of 17 .. 40 bits when the byte stream rides on the sort."""
    passes = (max(key_bits, 1) + 7) // 8
    if not (carry and pack and 3 <= passes <= 5 and n >= 65536):
        return "wide"
    return "split40" if key_bits > 32 else "split32"


def predict(mod, m, plan, tiles_knob=False, biglist_nomem=False, gather=False, pack=True, target=CHUNK_TARGET):
    """What a fresh context reports for fixed-width keys of m symbols (tests/forward_cases.py: the exact cells).  plan(a0, a_chunks, target)
    is bwts_debug_chunk_plan_target: ([S(a0), capacity, S(a_chunks), chunks of the re-cut], the re-cut fits); target is what
    BWTS_CHUNK_TARGET says.  The chunk count is held against the capacity wherever it grows: a run that the engine would end with
    "chunk table full" fails here first."""
    n = mod.n
    carry = mod.cyclic and not gather
    p = {"cyclic": mod.cyclic, "n": n, "k": mod.k, "need_sa": (not mod.cyclic) or gather, "flags_outside_rank": carry and n >= FLAGS_OUTSIDE_N}
    sigma = int(np.unique(mod.x).size)
    codes = sigma if mod.cyclic else sigma + 1                    # (the suffix form keeps code 0 for "past the end")
    p["sigma"], p["bits"] = sigma, max(codes - 1, 1).bit_length()
    p["msym"] = p["hstep"] = m
    p["key_bits"], p["varlen"] = p["bits"] * m, False
    p["keys"] = key_form(p["key_bits"], n, carry, pack)
    dlog = min(p["key_bits"], 20, n.bit_length())                 # the sparse form's key directory: needs 8 bits to index
    p["directory"] = dlog if dlog >= 8 else 0
    a0 = mod.stats(m)["tied"]
    p["tied0"] = a0
    p["rank_early"] = a0 > n // 32 and p["flags_outside_rank"] and n >= RANK_EARLY_N
    p["no_chunks"] = None
    if a0 == 0:
        p.update(form="none", end="none", rounds=1, round=[], round_active=[0], left=0, need_sa=False)
        return p
    if a0 <= n // 32:
        form = "sparse"
    elif tiles_knob:
        form, p["no_chunks"] = "tiles", "knob"
    elif a0 < CH_MIN_LIST:
        form, p["no_chunks"] = "tiles", "short_list"
    elif biglist_nomem and mod.stats(m)["mid"] + mod.stats(m)["huge"] > 0:
        form, p["no_chunks"] = "tiles", "no_room_biglist"
    else:
        form = "chunks"
    st, end = mod.walk(m, 2 if form == "sparse" else 4)
    p.update(form=form, end=end, rounds=len(st), round_active=[s["tied"] for s in st], left=st[-1]["tied"])
    if form == "sparse":
        p["need_sa"] = False                    # (the sparse form keeps the suffix array as it goes: nobody asks)
    rounds = []
    if form == "sparse":
        skip = False
        for r in range(1, len(st)):
            a, big = st[r - 1]["tied"], st[r - 1]["gt_seg"]
            rd = {"form": "sparse", "h": st[r - 1]["depth"], "in": a, "out": st[r]["tied"], "split": st[r]["classes"] > st[r - 1]["classes"]}
            if a <= SEG_MIN_LIST:
                rd.update(probe="short_list", m_big=0, whole=True, skip_next=False)
                skip = False
            elif skip:
                rd.update(probe="skipped", m_big=0, whole=True, skip_next=False)
                skip = False
            else:
                skip = big * 10 > a * 9
                rd.update(probe="ran", m_big=big, whole=big * 5 > a * 4, skip_next=skip)
            rounds.append(rd)
    elif form == "tiles":
        for r in range(1, len(st)):
            rounds.append({"form": "tiles", "h": st[r - 1]["depth"], "in": st[r - 1]["tied"], "out": st[r]["tied"],
                           "split": st[r]["classes"] > st[r - 1]["classes"], "m_big": st[r - 1]["mid"] + st[r - 1]["huge"]})
        p["order_sort"] = a0 >= CH_MIN_LIST
        p["rest_tiles"] = st[-1]["tied"] if end == "stable" else 0
    else:
        s0 = st[0]
        (S, cap, _, _), _ = plan(a0, a0, target)
        ch = {"S": S, "maxchunks": cap, "a_small": s0["le_cap"], "big0": s0["mid"] + s0["huge"], "fsl": mod.cyclic and mod.k <= CH_FS,
              "m_exit": 0, "m_stay": 0, "groups": 0, "compactions": 0, "compactions_skipped": 0, "enqueued_behind_last": False}
        S_recut, round_S = 0, []              # the nominal size after the last compaction, and as each round ran
        nchunks = -(-s0["le_cap"] // S)
        assert nchunks <= cap, ("the first cut", nchunks, cap)
        tail = a_chunks = s0["le_cap"]
        big = 0
        wide = False
        if ch["big0"]:
            ch.update(m_exit=s0["mid"], m_stay=s0["huge"], groups=s0["huge_groups"])
            if s0["mid"]:
                nchunks += -(-s0["mid"] // S); tail += s0["mid"]; a_chunks += s0["mid"]; wide = True
                assert nchunks <= cap, ("the first split", nchunks, cap)
            big = s0["huge"]
        r, finished = 1, False
        while not finished:
            B = 1 if big else 2
            for q in range(B):
                if finished:
                    ch["enqueued_behind_last"] = True
                    continue
                new = st[r]
                stays = new["huge"] if big else 0
                # what leaves the big list: its elements now in groups of 2 .. CH_GROUP_MAX (a group of the chunks never grows)
                leaves = (new["tied"] - stays - _still_tied_from_chunks(mod, st[r - 1]["depth"], new["depth"])) if big else 0
                in_chunks = new["tied"] - stays - leaves
                rounds.append({"form": "chunks", "h": st[r - 1]["depth"], "in": a_chunks + big, "out": new["tied"],
                               "split": new["classes"] > st[r - 1]["classes"], "chunks_in": a_chunks, "chunks_out": in_chunks, "big_in": big,
                               "big_stays": stays, "big_leaves": leaves, "nchunks": nchunks})
                round_S.append(S)
                if leaves:
                    nchunks += -(-leaves // S); tail += leaves; wide = True
                    assert nchunks <= cap and tail <= a0, ("an append", len(rounds), nchunks, cap, tail, a0)
                big = stays
                a_chunks = in_chunks + leaves
                r += 1
                if r == len(st):
                    finished = True
            if not finished and nchunks >= 64 and a_chunks > 0 and a_chunks * 3 < tail:
                (_, _, S2, nc), fits = plan(a0, a_chunks, target)
                assert fits and nc <= cap, ("a re-cut", a0, a_chunks, nc, cap)
                ch["compactions"] += 1
                S_recut = S2
                S, nchunks, tail = S2, nc, a_chunks
        ch["wide_possible"] = wide
        p["chunks"] = ch
        p["chunk_S_recut"], p["chunk_round_S"] = S_recut, round_S
        p["rest_chunks"] = a_chunks if end == "stable" and nchunks else 0
        p["rest_big"] = big if end == "stable" else 0
    p["round"] = rounds
    return p


def _still_tied_from_chunks(mod, d_old, d_new):
    """Elements that sat in chunks at depth d_old (tied, in groups of at most CH_GROUP_MAX) and are still tied at depth d_new."""
    old, new = mod.sizes(d_old), mod.sizes(d_new)
    return int(((old > 1) & (old <= CH_GROUP_MAX) & (new > 1)).sum())


def brute_classes(x, starts, d, cyclic=True):
    """Classes at depth d by writing the words out (small inputs only): the check of Model.classes."""
    n = len(x)
    words = []
    ends = list(starts[1:]) + [n] if cyclic else None
    for p in range(n):
        if cyclic:
            f = max(i for i, s in enumerate(starts) if s <= p)
            fs, fl = starts[f], ends[f] - starts[f]
            words.append(tuple(int(x[fs + (p - fs + j) % fl]) for j in range(d)))
        else:
            words.append(tuple(int(x[p + j]) if p + j < n else -1 for j in range(d)))
    order = {w: i for i, w in enumerate(sorted(set(words)))}
    return np.array([order[w] for w in words], dtype=np.int64)


def brute_lyndon_starts(x):
    """Factor starts by the definition: the longest prefix that is strictly smaller than all its proper suffixes, again and again."""
    b, out, i = bytes(x), [], 0
    while i < len(b):
        best = 1
        for L in range(1, len(b) - i + 1):
            w = b[i:i + L]
            if all(w < w[j:] for j in range(1, L)):
                best = L
        out.append(i)
        i += best
    return out
