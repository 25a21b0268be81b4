"""Round-0 keys from their definition, in numpy: no GPU, no engine code.

Three things, each written from what DESIGN.md and the comments of csrc/key_plan.h say a key IS, not from how the kernels build one.

1. optimal_alphabetic_cost(w): the least sum of w[i] * depth[i] over all binary trees whose leaves are the symbols in order, by the
   plain interval recurrence C[i][j] = W(i..j) + min over every k of C[i][k] + C[k+1][j] -- every split point is tried, there is no
   monotone-root bound.  The engine's weights hist[c] + (n >> 14) + 1 are integers, so every cost below 2^53 is exact in a double and
   the comparison with the library's code table is ==.

2. The key of every position from a code table.
   varlen_keys: the first key_bits bits of the concatenated code words of the rotation of p inside its own Lyndon factor (the word of
   x[p], of the position behind it, ... wrapping at the factor's end), most significant bit first, as a number of key_bits bits.
   fixed_keys: the first msym codes of bits bits each; the cyclic form wraps inside the factor, the suffix form reads zeros past n
   (its codes start at 1).
   Both walk one symbol step at a time for all positions at once; a key of 64 bits is full after at most 64 steps.

3. KeyModel(Model): the partitions of the sort's rounds from those keys.  After round 0 two positions are in one group exactly when
   their keys are equal.  A later round never looks at symbols again: it reads, for every tied position, the rank (group) of its
   successors as the round before left them, all of one version, and splits by the tuple.  Per form (forward_model.py):
     sparse     round r >= 1 reads one successor, at distance h = hstep * 2^(r-1): the groups after round r are the classes of
                (group after round r-1 at p, group after round r-1 at the h-th successor of p) -- classes(hstep * 2^r) below;
     chunks,    round r reads three successors, at h, 2h and 3h with h = hstep * 4^(r-1): classes(hstep * 4^r), which is the sparse
     tiles      form's partition of every second round;
     direct     one round that compares rotations symbol by symbol until they differ: nothing is left tied.
   hstep is the number of symbols EVERY key covers (key_bits // longest code word, at least 1; msym for fixed-width codes): the
   successor at distance hstep starts inside or right behind what the key of p has seen, never beyond a gap, so composing keys at
   distances hstep * 2^r loses no symbol.  Keys overlap (a key usually covers more than hstep symbols); that makes the classes finer
   than "first hstep * 2^r symbols", never coarser, and the model composes exactly what the engine composes.
   classes(d) is defined for d = hstep * u: depth a + b from depth a at p and depth b at the a-th successor, as Model.compose does.
   With classes() replaced, Model.walk / stats / sizes and forward_model.predict(mod, hstep, ...) give the rounds' tied counts;
   predict_keys() below puts the key's own header words in place of the fixed-width ones predict() writes."""
import numpy as np

import forward_model as M


def optimal_alphabetic_cost(w):
    """Least weighted path length of an alphabetic binary tree over the weights w (in symbol order): O(len^3), every split tried."""
    w = np.asarray(w, dtype=np.float64)
    s = w.size
    if s == 1:
        return 0.0
    pre = np.concatenate([[0.0], np.cumsum(w)])
    assert pre[-1] * s < 2.0 ** 53, "the sums must stay exact"
    C = np.zeros((s, s), dtype=np.float64)
    for L in range(2, s + 1):
        for i in range(0, s - L + 1):
            j = i + L - 1
            C[i, j] = (C[i, i:j] + C[i + 1:j + 1, j]).min() + (pre[j + 1] - pre[i])
    return float(C[0, s - 1])


def smoothed_weights(hist, n):
    """The weights the engine's code is optimal for: every present symbol's count plus n / 2^14 + 1."""
    h = np.asarray(hist, dtype=np.int64)
    return h[h > 0] + (int(n) >> 14) + 1


def _factor_of(x, starts):
    n = x.size
    lens = np.diff(np.append(starts, n))
    return np.repeat(starts, lens).astype(np.int64), np.repeat(lens, lens).astype(np.int64)


def varlen_keys(x, starts, vlen, vcode, key_bits):
    """The key of every position: the first key_bits bits of the code words of x[p], x[p+1], ... round and round p's Lyndon factor."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n = x.size
    fs, fl = _factor_of(x, np.asarray(starts, dtype=np.int64))
    off = np.arange(n, dtype=np.int64) - fs
    L = np.asarray(vlen, dtype=np.int64)[x]              # per position: its own word
    Cw = np.asarray(vcode, dtype=np.uint64)[x]
    assert L.min() >= 1 and 8 <= key_bits <= 64
    acc = np.zeros(n, dtype=np.uint64)
    filled = np.zeros(n, dtype=np.int64)
    for step in range(64):
        act = np.flatnonzero(filled < key_bits)
        if act.size == 0:
            break
        q = fs[act] + (off[act] + step) % fl[act]
        l, c, room = L[q], Cw[q], key_bits - filled[act]
        whole = l <= room
        take = np.where(whole, l, room)                                   # bits of this word that still fit: its leading ones
        acc[act] = (acc[act] << take.astype(np.uint64)) | (c >> (l - take).astype(np.uint64))
        filled[act] += take
    assert (filled == key_bits).all()
    return acc


def fixed_keys(x, starts, codes, bits, msym, pad_add=0):
    """Fixed-width keys: msym codes of `bits` bits.  starts: the Lyndon factors' starts (cyclic form), or None for the suffix form,
    which reads code 0 past the end (its table codes, plus pad_add, start at 1)."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n = x.size
    code = np.asarray(codes, dtype=np.uint64)[x] + np.uint64(pad_add)
    assert bits * msym <= 64 and int(code.max()) < (1 << bits)
    p = np.arange(n, dtype=np.int64)
    if starts is not None:
        fs, fl = _factor_of(x, np.asarray(starts, dtype=np.int64))
    else:
        code = np.append(code, np.uint64(0))
    acc = np.zeros(n, dtype=np.uint64)
    for step in range(msym):
        q = fs + (p - fs + step) % fl if starts is not None else np.minimum(p + step, n)
        acc = (acc << np.uint64(bits)) | code[q]
    return acc


def tied(keys):
    """Positions whose key some other position has too."""
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


def keys_of_plan(x, starts, plan):
    """The keys of a cyclic sort whose layout is `plan` (a dict of debug_key_plan)."""
    if plan["varlen"]:
        return varlen_keys(x, starts, plan["vlen"], plan["vcode"], plan["key_bits"])
    return fixed_keys(x, starts, plan["codes"], plan["bits"], plan["msym"], plan["pad_add"])


class KeyModel(M.Model):
    """The rounds of a sort whose round 0 made `keys` (one per position) and whose round 1 steps by hstep symbols (module docstring)."""

    def __init__(self, x, keys, hstep, cyclic=True):
        super().__init__(x, cyclic)
        self.hstep = int(hstep)
        assert self.hstep >= 1 and len(keys) == self.n
        _, inv = np.unique(np.asarray(keys), return_inverse=True)
        self._cls = {self.hstep: inv.astype(np.int64) + (0 if cyclic else 1)}
        self._stats = {}

    def classes(self, d):
        d = int(d)
        assert d >= self.hstep and d % self.hstep == 0, (d, self.hstep)
        if d not in self._cls:
            u = d // self.hstep
            a = (u - u // 2) * self.hstep
            self._cls[d] = self.compose(self.classes(a), a, self.classes(d - a))
        return self._cls[d]

    def final_tied(self, m=None):
        return self.walk(self.hstep, 2)[0][-1]["tied"]


def predict_keys(mod, plan, chunk_plan, **knobs):
    """forward_model.predict for a KeyModel: the rounds from the keys' classes, the header from the key's own layout."""
    p = M.predict(mod, mod.hstep, chunk_plan, **knobs)
    carry = mod.cyclic and not knobs.get("gather", False)
    kb = plan["key_bits"]
    p.update(msym=plan["msym"], hstep=plan["hstep"], key_bits=kb, varlen=plan["varlen"], bits=plan["bits"], sigma=plan["sigma"],
             keys=M.key_form(kb, mod.n, carry, knobs.get("pack", True)))
    dlog = min(kb, 20, mod.n.bit_length())
    p["directory"] = dlog if dlog >= 8 else 0
    return p
