"""A CPU model of the segmented inverse's shared pass -- test infrastructure only, plain numpy, written from the definition.

bwts_inverse_segments may send a run of consecutive segments through ONE splitter walk.  The pass builds LF per segment but with
indices of the whole run,

    LF[off_s + p] = off_s + C_s[B[p]] + occ_s(B[p], p)        (C_s, occ_s: of segment s alone)

a permutation of [0, n) whose cycles each lie inside one segment; everything the walk, the node ranking and the cycle order do
works on any permutation (inverse_model.Model, whose counts this class inherits unchanged).  Two rules are the segmented form's own:

  the symbol of x is read from the input, B[x] (one C table per segment: it cannot be looked up from LF[x] in a shared table);
  a cycle with smallest element m in segment s (off[s] <= m < off[s + 1]) ends at  off[s + 1] - 1 - (used - off[s]),  `used` the
  summed lengths of the cycles ordered before it by smallest element: the cycles of earlier segments come first and sum to off[s].

inverse() applies both, one cycle at a time (unbwts.c:62-86 per segment, restated on the shared permutation)."""
import numpy as np

import inverse_model as M


def bounds(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=off[1:])
    return off


def segment_lf_map(B, lengths):
    """The per-segment stable LF map with global indices: rank of i in a stable sort by (segment, byte)."""
    B = np.ascontiguousarray(B, dtype=np.uint8)
    off = bounds(lengths)
    assert off[-1] == B.size
    seg = np.repeat(np.arange(len(lengths), dtype=np.int64), np.asarray(lengths, dtype=np.int64))
    order = np.argsort(seg * 256 + B, kind="stable")
    LF = np.empty(B.size, dtype=np.int64)
    LF[order] = np.arange(B.size, dtype=np.int64)
    return LF


class SegmentModel(M.Model):
    """inverse_model.Model over the shared pass's permutation: at(g), class_deficits, wrap_points and predict() apply as they are."""

    def __init__(self, B, lengths):
        self.B = np.ascontiguousarray(B, dtype=np.uint8)
        self.n = n = self.B.size
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.off = bounds(self.lengths)
        self.LF = segment_lf_map(self.B, self.lengths)
        m, p, span = np.arange(n, dtype=np.int64), self.LF.copy(), 1
        while span < n:
            m = np.minimum(m, m[p])
            p = p[p]
            span *= 2
        self.cmin = m
        self.cycles = int(np.count_nonzero(m == np.arange(n)))
        self._at, self._un = {}, {}

    def segment_of(self, x):
        return int(np.searchsorted(self.off, x, side="right")) - 1

    def inverse(self):
        """The text of every segment, by the two rules of the shared pass."""
        n, B, off, lf = self.n, self.B, self.off, self.LF.tolist()
        assert np.array_equal(np.searchsorted(off, self.LF, side="right"), np.searchsorted(off, np.arange(n), side="right")), \
            "a cycle crosses a segment boundary"
        out = np.zeros(n, dtype=np.uint8)
        written = np.zeros(n, dtype=bool)
        used = 0
        for m in np.nonzero(self.cmin == np.arange(n))[0].tolist():        # the cycles by smallest element
            xs, x = [m], lf[m]
            while x != m:
                xs.append(x)
                x = lf[x]
            s = self.segment_of(m)
            end = int(off[s + 1]) - 1 - (used - int(off[s]))
            pos = end - np.arange(len(xs))
            assert off[s] <= pos[-1] and not written[pos].any()
            out[pos] = B[xs]                                                # out[end - t] = B[LF^t(m)]
            written[pos] = True
            used += len(xs)
        assert used == n and written.all()
        return out
