"""CPU suite: the model of the inverse's splitter walk (tests/inverse_model.py) against the oracle and brute force, the numbers
it was introduced with, and the condition tests/test_inverse_paths.py rests on: the built inputs reach every path on its coverage
list by the model's prediction alone."""
import numpy as np
import pytest

import inverse_cases as IC
import inverse_model as M
import oracle_lib as O


def _brute(B, g):
    """Cycle by cycle, the way unbwts.c:66-86 walks them."""
    LF = M.lf_map(B).tolist()
    n, G = len(LF), 1 << g
    seen, cycles, unreached, longest = [False] * n, 0, 0, 0
    for i in range(n):
        if seen[i]:
            continue
        cyc, x = [], i
        while not seen[x]:
            seen[x] = True
            cyc.append(x)
            x = LF[x]
        cycles += 1
        if not any(y % G == 0 for y in cyc):
            unreached += len(cyc)
            longest = max(longest, len(cyc))
    return cycles, unreached, longest


@pytest.mark.parametrize("seed", range(12))
def test_model_vs_brute_force_and_oracle(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 3000))
    B = rng.integers(0, int(rng.choice([1, 2, 3, 7, 256])), size=n, dtype=np.uint8)
    if seed % 3 == 0:
        B = np.sort(B)
    mod = M.Model(B)
    assert mod.cycles == len(O.lyndon_starts(O.inverse(B)))
    for g in (0, 1, 2, 4, 6):
        r = mod.at(g)
        assert (r["cycles"], r["unreached"], r["longest"]) == _brute(B, g), (seed, g)
        assert r["nu2_lo"] <= r["nu2_hi"]


def test_model_virtual_nodes_by_hand():
    """A single cycle 0 -> 1 -> ... -> n-1 -> 0 (B = 1^(n-1) 0: LF is i + 1 mod n) at g = 2: stretches of 4 steps, slot 16, no cut.
    i -> i + 3 mod 64 at g = 4: the walk from 0 meets 48 after 16 steps -- exactly a slot: it closes there, no virtual node."""
    r = M.Model(IC.rotation(64, 1)).at(2)
    assert (r["cycles"], r["unreached"], r["virtual"], r["max_stretch"]) == (1, 0, 0, 4)
    mod = M.Model(IC.rotation(64, 3))
    r = mod.at(2)            # slot 16; from 0: 3, 6, 9, 12 -> 4 steps
    assert r["virtual"] == 0 and r["max_stretch"] == 4
    r = mod.at(4)            # slot 64
    assert (r["s"], r["virtual"], r["unreached"]) == (4, 0, 0) and r["max_stretch"] == 16
    # 1^(n-c) 0^c with n = 97, c = 16 at g = 4 (slot 64, splitters 0, 16, ..., 96): one cycle (97 is prime); the index changes its
    # residue mod 16 only when the walk wraps: 0 -> 16 -> ... -> 96 are stretches of 1, then 96 -> 15 -> 31 ... stays off the
    # splitters for 15 wraps of 6 steps each, + 1: a stretch of 91 steps, one cut
    r = M.Model(IC.rotation(97, 16)).at(4)
    assert (r["cycles"], r["unreached"], r["virtual"], r["max_stretch"]) == (1, 0, 1, 91)


def test_model_wrap_points():
    """i -> i + 1 mod 40 at g = 3 (slot 32): nodes start at 0, 8, .., 32 with 8 symbols each; the walk from x reaches element 0
    after 40 - x steps."""
    w = M.Model(IC.rotation(40, 1)).wrap_points(3)
    assert w == [(8, 40), (8, 32), (8, 24), (8, 16), (8, 8)]
    w = M.Model(IC.rotation(97, 16)).wrap_points(4)
    # the stretch from 96 is cut after 64 steps; nodes: 0, 16, .., 80 (1 step each), 96 (64), the virtual node (27)
    assert sorted(l for l, _ in w) == [1] * 6 + [27, 64]
    assert sum(l for l, _ in w) == 97


@pytest.mark.parametrize("c,g,s,virtual,room,overflow", [(16 * 164, 4, 16385, 3772, 3072, True), (16000, 4, 16385, 3000, 3072, False),
                                                         (64 * 41, 6, 4097, 984, 1536, False), (256 * 11, 8, 1025, 253, 1152, False)])
def test_model_reproduces_the_rotation_numbers(c, g, s, virtual, room, overflow):
    r = M.Model(IC.rotation(IC.ROT_N, c)).at(g)
    assert (r["s"], r["virtual"], r["room"], r["overflow"]) == (s, virtual, room, overflow)


def test_model_long_cycles_without_a_splitter():
    r = M.Model(IC.rotation(1 << 18, 32 * 1001)).at(4)
    assert (r["cycles"], r["unreached"], r["longest"], r["virtual"]) == (32, 245760, 8192, 0)
    assert r["nu2_lo"] == r["nu2_hi"] == 8192            # the class = 16 mod 32: all splitters, node ids odd
    r = M.Model(IC.rotation(1 << 18, 2 * 25001)).at(4)
    assert (r["cycles"], r["unreached"], r["longest"]) == (2, 1 << 17, 1 << 17)


_models = {}


def _chains():
    """case name -> {(g, mark): predicted chain}, every cell of the GPU file."""
    if not _models:
        for case in IC.CASES:
            mod = M.Model(case.build())
            _models[case.name] = {(g, m): M.predict(mod, g, m) for c, g, m, _ in IC.ALL_CELLS if c is case}
    return _models


def test_case_names_are_unique_and_sizes_bounded():
    names = [c.name for c in IC.CASES]
    assert len(set(names)) == len(names)
    assert {(g, m) for _, g, m, _ in IC.ALL_CELLS} == {(g, m) for g in IC.G_MATRIX for m in IC.MARKS}


def test_every_path_is_predicted():
    """What the GPU file's last test demands of the engine's reports, the model predicts for the same cells: the inputs are built
    for it.  And every tag of a case holds in the prediction for its home cells."""
    seen = set()
    for case in IC.CASES:
        for (g, mark), chain in _chains()[case.name].items():
            seen |= IC.coverage_of(chain)
            if g in case.homes:
                for tag in case.tags:
                    assert IC.tag_holds(tag, chain, mark) in (True, None), (case.name, g, mark, tag, chain)
    assert not [c for c in IC.COVERAGE if c not in seen], sorted(seen)


def test_moments_replay_by_hand():
    """n = 4096 sorted bytes at g = 4: every class (mod 1024) whose index is no multiple of 16 misses all four of its elements:
    960 classes listed, nothing named, all chased (cycles of one element).  n = 2048: they miss two each, named by arithmetic."""
    assert M.moments_route(M.Model(np.zeros(4096, np.uint8)), 4) == dict(route="search", listed=960, fallback=False, cycle_passes=0)
    assert M.moments_route(M.Model(np.zeros(2048, np.uint8)), 4) == dict(route="arithmetic", listed=0, fallback=False, cycle_passes=0)
    # two cycles of 2^17 elements, the odd one unreached: 512 classes miss all 256 of theirs, and the chase cannot follow such a cycle
    assert M.moments_route(M.Model(IC.rotation(1 << 18, 2 * 25001)), 4) == dict(route="need_log", listed=512, fallback=True, cycle_passes=0)
    # a constant input of 6 Mi: 960 classes of 6144 elements are more than the search may look at
    assert M.moments_route(M.Model(np.full(6 << 20, 7, np.uint8)), 4) == dict(route="need_log", listed=0, fallback=True, cycle_passes=0)


def test_wrap_cases_meet_every_branch_of_the_placement():
    """g >= 5: 2^(g-4) threads share a node, thread `sub` moving the 16-symbol chunks sub, sub + tpn, ...  The chunk test of
    place_segments_kernel compares the wrap point wr with the chunk's bounds c and c + 16 only (c a multiple of 16), so what a chunk
    does depends on wr through wr mod 16 and on which chunk holds it: wr = 16 and wr = 17 behave as 0 and 1 one chunk later.  Over
    the wrap cases the model finds, for EVERY g of 5, 6, 8, 12, nodes of two chunks or more whose wrap point falls inside them at
    offsets 0, 1 and 15 of a chunk (0: the two clean branches side by side; 1, 15: the straddling chunk, byte by byte), such a
    chunk owned by a thread other than sub 0, nodes the wrap point lies behind (wr >= len), and cycles of 16 k + r elements for
    r = 0, 1, 15."""
    offsets, lengths, other_thread, behind = set(), set(), set(), set()
    for case in IC.CASES:
        if case.name not in IC.WRAP_CASES:
            continue
        mod = M.Model(case.build())
        lengths |= {int(v) % 16 for v in np.bincount(mod.cmin)[np.bincount(mod.cmin) > 0]}
        for g in (5, 6, 8, 12):
            tpn = 1 << (g - 4)
            for ln, wr in mod.wrap_points(g):
                if ln >= 32 and 0 < wr < ln:
                    offsets.add((g, wr % 16))
                    if (wr // 16) % tpn:
                        other_thread.add(g)
                elif ln >= 32:
                    behind.add(g)
    assert {0, 1, 15} <= lengths
    assert {(g, o) for g in (5, 6, 8, 12) for o in (0, 1, 15)} <= offsets, sorted(offsets)
    assert other_thread == behind == {5, 6, 8, 12}
