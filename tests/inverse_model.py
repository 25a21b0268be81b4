"""A CPU model of the inverse's splitter walk -- test infrastructure only, plain numpy, written from the definition.

The inverse follows LF (unbwts.c:50-52: LF[i] = rank of i in a stable sort of B) from every 2^g-th index -- the splitters -- to the
next splitter, all walks at once.  What the engine reports about one attempt (Context.debug_inverse_report) is a function of B and g
alone, and this model computes it the slow way:

  cycles      LF cycles (= Lyndon factors of the text)
  unreached   elements in cycles that hold no splitter; `longest`: the longest such cycle
  virtual     a splitter-to-splitter stretch of l steps is cut every `slot` steps: (l - 1) // slot cuts (a walk that stands on a
              splitter at exactly `slot` steps closes there), each a virtual node
  overflow    more virtual nodes than the node pool has room for
  nu2         nodes of the reduced list on node cycles that hold no level-2 splitter (node id = 0 mod 32).  Splitter x has node
              id x >> g; virtual nodes get their ids from an atomic counter, so a node cycle with virtual nodes and no level-2
              splitter among its splitter nodes is undecided: nu2 is given as a range (nu2_lo, nu2_hi), equal where no such
              cycle exists

Three constants are shared with inverse.hip, because the counts are defined in their terms: splitters are the indices = 0 mod
2^g; slot = max(16, 4 * 2^g); node_cap = s + s/8 + 1024 (s at g = 0, where no stretch is longer than one step); and L2_H = 32 for
the level-2 rule.  predict() below is a second, separate layer: which branch the engine's host code takes for such counts, from the
thresholds that host code states (UNV_CAP0, one_lane_cap, the chase's step cap, the moments' budget)."""
import numpy as np

L2_H = 32


def lf_map(B):
    B = np.ascontiguousarray(B, dtype=np.uint8)
    order = np.argsort(B, kind="stable")
    LF = np.empty(B.size, dtype=np.int64)
    LF[order] = np.arange(B.size, dtype=np.int64)
    return LF


def slot_of(g):
    return max(16, 4 << g)


def node_room(n, g):
    """node_cap - s: virtual nodes the pool has room for."""
    s = (n + (1 << g) - 1) >> g
    return 0 if g == 0 else s // 8 + 1024


class Model:
    def __init__(self, B):
        self.B = np.ascontiguousarray(B, dtype=np.uint8)
        self.n = n = self.B.size
        self.LF = lf_map(self.B)
        # smallest element of every element's cycle: after r rounds m[x] = min of x, LF x, ..., LF^(2^r - 1) x
        m, p, span = np.arange(n, dtype=np.int64), self.LF.copy(), 1
        while span < n:
            m = np.minimum(m, m[p])
            p = p[p]
            span *= 2
        self.cmin = m
        self.cycles = int(np.count_nonzero(m == np.arange(n)))
        self._at, self._un = {}, {}

    def at(self, g):
        """The counts of one attempt with splitter spacing 2^g."""
        if g in self._at:
            return self._at[g]
        n, LF, G = self.n, self.LF, 1 << g
        start = np.arange(0, n, G, dtype=np.int64)
        s, slot, room = start.size, slot_of(g), node_room(n, g)
        visited = np.zeros(n, dtype=bool)
        steps = np.zeros(s, dtype=np.int64)
        alive, cur = np.arange(s), start.copy()
        while alive.size:                         # all walks advanced together, one step at a time
            visited[cur] = True
            cur = LF[cur]
            steps[alive] += 1
            on = (cur & (G - 1)) != 0
            alive, cur = alive[on], cur[on]
        cuts = (steps - 1) // slot
        virtual = int(cuts.sum())
        un = ~visited
        unreached = int(np.count_nonzero(un))
        longest = 0
        if unreached:
            longest = int(np.bincount(self.cmin[un]).max())
        # level 2: the node cycle of an LF cycle is made of its splitters' nodes and their virtual nodes
        _, inv = np.unique(self.cmin[start], return_inverse=True)
        has_l2 = np.bincount(inv, weights=(np.arange(s) % L2_H == 0)) > 0
        has_virtual = np.bincount(inv, weights=cuts) > 0
        nodes = np.bincount(inv) + np.bincount(inv, weights=cuts).astype(np.int64)
        nu2_lo = int(nodes[~has_l2 & ~has_virtual].sum())
        nu2_hi = nu2_lo + int(nodes[~has_l2 & has_virtual].sum())
        r = dict(g=g, n=n, s=s, slot=slot, cycles=self.cycles, unreached=unreached, longest=longest, virtual=virtual, room=room,
                 overflow=virtual > room, nu2_lo=nu2_lo, nu2_hi=nu2_hi, max_stretch=int(steps.max()),
                 unreached_cycles=int(np.count_nonzero(un & (self.cmin == np.arange(n)))))
        self._at[g] = r
        self._un[g] = un
        return r

    def class_deficits(self, g, shift):
        """Per residue class of the index mod 2^shift: how many of its elements no walk reached."""
        self.at(g)
        un = self._un[g]
        return np.bincount(np.nonzero(un)[0] & ((1 << shift) - 1), minlength=1 << shift)

    def wrap_points(self, g):
        """Per node of the reduced list (virtual nodes included), for the placement: (len, wrap) -- the symbols the node recorded
        and how many of them come before the walk passes its cycle's smallest element (wrap >= len: not inside this node)."""
        n, LF, G, slot = self.n, self.LF, 1 << g, slot_of(g)
        # to_min[x] = steps from x until the walk stands on its cycle's smallest element (a whole cycle from that element itself)
        is_min = self.cmin == np.arange(n)
        dist = np.ones(n, dtype=np.int64)
        hop = LF.copy()
        done = is_min[hop]
        span = 1
        while span < n:
            go = np.nonzero(~done)[0]
            if go.size == 0:
                break
            h = hop[go]
            dist[go] += dist[h]
            done[go] = done[h]
            hop[go] = hop[h]
            span *= 2
        out, lf = [], LF.tolist()
        for x0 in range(0, n, G):
            x, ln = x0, 0                         # the stretch from x0, cut every `slot` steps
            while True:
                y = lf[x]
                ln += 1
                if y & (G - 1) == 0 or ln == slot:
                    out.append((ln, int(dist[x0])))
                    if y & (G - 1) == 0:
                        break
                    x0, ln = y, 0
                x = y
        return out


# ---- which branch the host code takes for such counts ---------------------------------------------------------------------------
UNV_CAP0 = 1 << 20            # room for unreached elements before their number is known (fresh context)
CHASE_CAP = 1 << 16           # steps one element of a listed class may chase before the moments give up
MOM_SHIFT = 10                # residue classes of the moments up to n = 2^30
MOM_BUDGET = 4 << 20          # elements the search of the listed classes may look at


def one_lane_cap(nu, G):
    cap = (1 << 36) // nu
    return 64 * G if cap > 64 * G else 4 * G if cap < 4 * G else cap


def predict(model, g, mark):
    """The chain of attempts a FRESH context makes for (g, mark): a list of dicts with g, mark, outcome, virtual, overflow, for a
    moments attempt `moments` (moments_route) and, for the attempt that finishes, nu2 (at least), second_collect and unit_rank."""
    chain = []
    n = model.n
    dense = False
    while True:
        r = model.at(g)
        a = dict(g=g, mark=mark, outcome="DONE", virtual=r["virtual"], overflow=r["overflow"])
        chain.append(a)
        if r["overflow"]:
            assert not dense
            a["outcome"] = "RETRY_DENSE"
            dense, g = True, 0
            if mark in ("log", "moments"):
                mark = "sentinel"
            continue
        if mark == "moments":
            a["moments"] = moments_route(model, g)
            if a["moments"]["fallback"]:
                a["outcome"] = "NEED_LOG"
                mark = "log"
                continue
        a["nu2"] = r["nu2_lo"]                  # (at least: see nu2 above)
        a["second_collect"] = r["unreached"] > min(n, UNV_CAP0)
        a["unit_rank"] = r["unreached"] > 0 and r["longest"] > one_lane_cap(r["unreached"], 1 << g)
        return chain


MOM_PASSES = 3                # looks at the classes in which the arithmetic may name one or two missing elements


def moments_route(model, g):
    """What the moments make of the elements no walk reached, replayed from the rules moments_resolve_kernel, moments_budget_kernel
    and moments_chase_kernel state (inverse.hip) on the model's own set of unreached elements -- every step is decided by that set:
      up to MOM_PASSES times: a class (index mod 2^MOM_SHIFT) still open that misses nothing is closed; one that misses one or
      two elements names them and is closed; one that misses more is listed and stays open.  Nothing listed: done.  Else every
      cycle that holds an element named in this pass hands its elements in open classes to the list (they no longer count as
      missing) -- a cycle of more than CHASE_CAP + 1 elements cannot be followed: the moments give up.
      then: the open classes that still miss something are listed; more than the budget's worth of elements in them: give up;
      else every element of a listed class is chased, and an unreached cycle of more than CHASE_CAP + 1 elements gives up.
    Returns dict(route, listed, fallback, cycle_passes): route 'none' (nothing unreached), 'arithmetic' (named by the classes'
    sums alone), 'cycles' (... and by the cycles of what was named), 'search' (classes listed and chased), 'need_log' (gave up);
    listed = classes listed when the search starts (0 after the budget refuses them)."""
    r = model.at(g)
    if r["unreached"] == 0:
        return dict(route="none", listed=0, fallback=False, cycle_passes=0)
    classes = 1 << MOM_SHIFT
    idx = np.nonzero(model._un[g])[0]
    cls = idx & (classes - 1)
    _, cyc = np.unique(model.cmin[idx], return_inverse=True)
    cyc_len = np.bincount(cyc)
    found = np.zeros(idx.size, dtype=bool)
    is_open = np.ones(classes, dtype=bool)
    fallback, cycle_passes, listed = False, 0, 0
    for p in range(1, MOM_PASSES + 1):
        d = np.bincount(cls[~found], minlength=classes)
        named_cls = is_open & ((d == 1) | (d == 2))
        is_open &= d > 2                              # complete and named classes are closed; the others are listed
        listed = int(np.count_nonzero(is_open))
        new = ~found & named_cls[cls]
        found |= new
        if listed == 0:
            break
        if not new.any():
            continue
        walked = np.zeros(cyc_len.size, dtype=bool)
        walked[cyc[new]] = True
        if np.any(cyc_len[walked] - 1 > CHASE_CAP):
            fallback = True
            break
        add = ~found & walked[cyc] & is_open[cls]
        if add.any():
            cycle_passes += 1
        found |= add
    else:
        d = np.bincount(cls[~found], minlength=classes)
        is_open &= d > 0
        listed = int(np.count_nonzero(is_open))
    if fallback:
        return dict(route="need_log", listed=listed, fallback=True, cycle_passes=cycle_passes)
    if listed == 0:
        return dict(route="cycles" if cycle_passes else "arithmetic", listed=0, fallback=False, cycle_passes=cycle_passes)
    per_class = (model.n + classes - 1) >> MOM_SHIFT
    if listed * per_class > max(MOM_BUDGET, per_class):
        return dict(route="need_log", listed=0, fallback=True, cycle_passes=cycle_passes)
    chased = ~found & is_open[cls]
    if np.any(cyc_len[cyc[chased]] - 1 > CHASE_CAP) or r["max_stretch"] > CHASE_CAP:
        return dict(route="need_log", listed=listed, fallback=True, cycle_passes=cycle_passes)
    return dict(route="search", listed=listed, fallback=False, cycle_passes=cycle_passes)
