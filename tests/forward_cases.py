"""Built inputs for the stages of the forward's sort (tests/test_forward_paths.py on the GPU, tests/test_forward_model.py on the CPU).

A case = one input, the key width m of its exact cell (fixed-width keys: BWTS_VARLEN=0 BWTS_KEY_SYMBOLS=m), the knobs of that cell, the
sort it looks at ("cyclic": Context.forward; "suffix": Context.debug_suffix_array; "general": Context.forward under BWTS_LYNDON=general,
which reports the suffix sort and then the cyclic one) and the path names it is there for.  A path name is checked twice: on the CPU
against forward_model.predict (so the coverage list is a condition the inputs meet by construction) and on the GPU against the engine's
report (Context.debug_forward_report).  Every cyclic input also runs once with no key knob: the default heuristics pick the key, and the
looser rules for any key apply (test_forward_paths.check_any_key).

COVERAGE: what each name means.
  round0.wide / split32 / split40   how round 0 keeps its keys: one u64 each (here by BWTS_RX_PACK=0 and by keys of more than 40 bits), split
                                    without / with the high byte
  round0.flags_carry / flags_rank   the group flags lie in the carried-byte buffers / in sp.rank (n < 4096, and BWTS_EMIT=gather)
  round0.nothing_tied               no later round
  sparse.no_probe                   a list of at most 4096: sorted whole
  sparse.probe_small_only           the probe ran and found no group of more than 8
  sparse.probe_compacted            ... found some, less than 4/5 of the list: compacted, sorted, written back
  sparse.whole                      ... found 4/5 or more: everything sorted
  sparse.skip_next                  more than 9/10: the next round has no probe
  sparse.directory / no_directory   the key directory exists / does not (fewer than 8 bits to index)
  sparse.ends_empty / ends_stable
  early_ranks.on / off              the dense ranks are built before the tied list (n >= 2^22, more than n/32 tied) / not, at 2^22 - 1
  chunks.fsl / general              factor starts in LDS (k <= 256) / the general-arithmetic instantiation
  chunks.small_only                 no group of more than 256: no big list
  chunks.biglist_leaves_at_once     a big list of groups of 257 .. 2048 only: it is empty after its first split
  chunks.biglist_drains             groups of more than 2048 stay, and pieces leave over more than one round
  chunks.biglist_at_stable_end      the big list still holds elements when no group splits any more (DgRest on the big list)
  chunks.wide                       WIDE chunks exist
  chunks.stable_rest                the stable finish lays out elements left in chunks
  chunks.ends_empty
  chunks.two_rounds_per_trip        a round was enqueued behind the last one
  chunks.compaction_done
  chunks.recut_smaller              a compaction re-cut the list at a nominal chunk size below the first cut's
  chunks.appends_after_recut        ... and a later round appended what left the big list, cut by that smaller size
  chunks.outgrows_first_cut         ... until the tables held more chunks than the first cut and first split made plus one per cut since:
                                    impossible at one nominal size, so the tables grew past what the first cut sizes
  handover.short_list / knob / no_room_biglist    why the tile form ran instead of chunks
  tiles.no_order_sort / order_sort  list below / from 65 536 elements
  tiles.big_groups / small_only     a round saw groups of more than 256 / none did
  tiles.stable_rest / ends_empty
  suffix.sparse / chunks_biglist / tiles          the suffix form (doubling_sort<false>) in each form of the later rounds
  general.sparse / chunks / tiles                 the same inside a forward under BWTS_LYNDON=general

Out of scope, kept by the 1 GiB goldens and the wide tests: n > 2^30 (sbits = 24 in early_ranks) and everything in wide_path.h.
"no room for the store" and "no room for the order block" need the device to be out of memory and stay out as well."""
import numpy as np

# The three names above need a nominal size that falls, and chunk_nominal_size is 2048 (its floor) from the start for every list below
# about 32 Mi elements.  BWTS_CHUNK_TARGET=64 (cuts aim at 64 chunks instead of 16 384) brings that arithmetic to test size: a list of
# 1 Mi elements or more starts at 16 384 and a re-cut of what is left lands lower.  This is the shape of the list that used to end in
# "chunk table full" (254 M elements cut at 16 384, re-cut at 2048, then 30 M elements leaving the big list); that input itself is
# tests/test_chunk_tables_gpu.py.  The chunk count of every round is part of the report that each cell holds against the model, and
# the model holds it against the tables' capacity (forward_model.predict).
CHUNK_TARGET_64 = {"BWTS_CHUNK_TARGET": "64"}


def noise(n, sigma, seed, base=0):
    return (np.random.default_rng(seed).integers(0, sigma, size=n, dtype=np.uint8) + np.uint8(base))


def pasted(n, sigma, seed, phrases):
    """Noise with phrases pasted in: phrases = [(length, times)]."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, sigma, size=n, dtype=np.uint8)
    for L, times in phrases:
        ph = rng.integers(0, sigma, size=L, dtype=np.uint8)
        for at in rng.integers(0, n - L, size=times):
            x[at:at + L] = ph
    return x


def twice(block):
    return np.concatenate([block, block])


def equal_factors_in_noise(n, length, seed):
    """Noise over 101 .. 255 (its factors all start above 100), a Lyndon word w = 100 + larger letters twice, then one long factor that
    starts with its only 50: the factors are the noise's, w, w and the tail -- two equal factors, 2 * length elements tied for ever."""
    rng = np.random.default_rng(seed)
    w = np.concatenate([[100], rng.integers(101, 256, length - 1)]).astype(np.uint8)
    head = rng.integers(101, 256, (n - 2 * length) // 2, dtype=np.uint8)
    tail = np.concatenate([[50], rng.integers(51, 256, n - 2 * length - head.size - 1)]).astype(np.uint8)
    return np.concatenate([head, w, w, tail])


def many_factors_twice(blocks, length, seed):
    """`blocks` Lyndon words with falling first letters, each there twice: 2 * blocks factors, every position tied for ever."""
    rng = np.random.default_rng(seed)
    parts = []
    for c in range(blocks - 1, -1, -1):
        w = np.concatenate([[c], rng.integers(c + 1, min(c + 6, 256), length - 1)]).astype(np.uint8)
        parts += [w, w]
    return np.concatenate(parts)


def factor_many_times(length, times, tail, seed):
    """A Lyndon word repeated `times` times, then one long smaller factor."""
    rng = np.random.default_rng(seed)
    w = np.concatenate([[10], rng.integers(11, 40, length - 1)]).astype(np.uint8)
    t = np.concatenate([[3], rng.integers(4, 40, tail - 1)]).astype(np.uint8)
    return np.concatenate([np.tile(w, times), t])


def variants(n, sigma, seed, lp, lq, kinds, times):
    """A phrase P followed by one of `kinds` tails, pasted `times` times in all: the group of P's positions is cut into `kinds` pieces
    once the depth reaches the tails."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, sigma, size=n, dtype=np.uint8)
    P = rng.integers(0, sigma, size=lp, dtype=np.uint8)
    Q = [rng.integers(0, sigma, size=lq, dtype=np.uint8) for _ in range(kinds)]
    slots = rng.permutation(n // (lp + lq + 8))[:times] * (lp + lq + 8)
    for i, at in enumerate(slots):
        ph = np.concatenate([P, Q[i % kinds]])
        x[at:at + ph.size] = ph
    return x


def two_level(n, seed, n_noise, lp, lq, kinds, times):
    """Noise over four letters; behind the first n_noise positions a phrase P of lp letters followed by one of `kinds` tails of lq
    letters, pasted `times` times.  With times > 2048 >= times / kinds the positions of P sit in the big list until the depth reaches
    their tail, and then leave it in groups of times / kinds that stay tied while the depth stays inside the tail: a round of depth d
    moves about min(lq, 3 d / 4) * times elements from the big list to the chunks, round after round, while the noise in front (tied
    in small groups at first, settled one round later) has emptied the chunks it was cut into."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, size=n, dtype=np.uint8)
    P = rng.integers(0, 4, size=lp, dtype=np.uint8)
    Q = [rng.integers(0, 4, size=lq, dtype=np.uint8) for _ in range(kinds)]
    slot = lp + lq + 8
    slots = n_noise + rng.permutation((n - n_noise) // slot)[:times] * slot
    for i, at in enumerate(slots):
        ph = np.concatenate([P, Q[i % kinds]])
        x[at:at + ph.size] = ph
    return x


def one_pair(n):
    x = np.arange(n, dtype=np.uint8)[::-1].copy()
    x[n // 2] = x[5]
    return x


class Case:
    def __init__(self, name, build, m, tags, sort="cyclic", env=None):
        self.name, self.build, self.m, self.tags, self.sort, self.env = name, build, m, tuple(tags), sort, dict(env or {})

    def __repr__(self):
        return self.name


_dense4 = lambda: np.concatenate([noise(1 << 20, 4, 11), twice(noise(1 << 14, 4, 12))])
_hundreds = lambda: np.concatenate([twice(noise(1 << 16, 256, 21)), pasted(1 << 17, 4, 22, [(48, 1000), (40, 700)])])
_drain = lambda: variants(1 << 20, 4, 31, 40, 40, 4, 6000)
_early = lambda n: pasted(n, 4, 41, [(64, 4096)])
# target 64: a0 = 2 097 152 cut at 16 384 (75 chunks), re-cut after round 1 at 3072 (46 chunks), 2218 elements appended in round 2
_recut = lambda: variants(1 << 21, 4, 31, 40, 40, 4, 12000)
# target 64: a0 = 2 621 440 cut at 16 384 (64 chunks, 70 with the first split), re-cut after round 1 at 2048 (56 chunks), then 103 352 and
# 116 024 elements appended in rounds 2 and 3: 164 chunks in round 4, 2.3 times what the first cut and split made
_recut_drain = lambda: two_level(5 << 19, 32, 1000000, 660, 40, 2, 2250)

CASES = [
    Case("noise256-m8", lambda: noise(1 << 17, 256, 1), 8, ["round0.wide", "round0.nothing_tied", "round0.flags_carry"]),
    Case("noise4-m13-n2p18", lambda: noise(1 << 18, 4, 2), 13, ["round0.split32", "sparse.no_probe", "sparse.directory", "sparse.ends_empty"]),
    Case("noise4-m13-n2p20", lambda: noise(1 << 20, 4, 3), 13, ["sparse.probe_small_only"]),
    Case("noise4-m20-n2p17", lambda: noise(1 << 17, 4, 4), 20, ["round0.split40"]),
    Case("phrase200-m13", lambda: pasted(1 << 20, 4, 5, [(40, 200)]), 13, ["sparse.probe_compacted"]),
    Case("phrase200-m16", lambda: pasted(1 << 20, 4, 6, [(60, 200)]), 16, ["sparse.whole", "sparse.skip_next"]),
    Case("one-pair-n120", lambda: one_pair(120), 1, ["sparse.no_directory", "round0.flags_rank"]),
    Case("equal-factors-in-noise", lambda: equal_factors_in_noise(1 << 17, 300, 7), 4, ["sparse.ends_stable"]),
    Case("early-on", lambda: _early(1 << 22), 8, ["early_ranks.on", "chunks.biglist_drains"]),
    Case("early-off", lambda: _early((1 << 22) - 1), 8, ["early_ranks.off"]),
    Case("dense4", _dense4, 8, ["chunks.fsl", "chunks.small_only", "chunks.compaction_done"]),
    Case("pairs-twice", lambda: twice(noise(1 << 17, 256, 8)), 5, ["chunks.small_only", "chunks.two_rounds_per_trip"]),
    Case("hundreds", _hundreds, 4, ["chunks.biglist_leaves_at_once", "chunks.wide"]),
    Case("drain", _drain, 8, ["chunks.biglist_drains", "chunks.wide", "chunks.ends_empty"]),
    Case("factor-3000-times", lambda: factor_many_times(30, 3000, 5000, 9), 4, ["chunks.biglist_at_stable_end"]),
    Case("many-factors-twice", lambda: many_factors_twice(250, 300, 10), 4, ["chunks.general", "chunks.stable_rest"]),
    Case("short-list", lambda: np.concatenate([noise(1 << 18, 256, 13), twice(noise(1 << 13, 256, 14))]), 4,
         ["handover.short_list", "tiles.no_order_sort", "tiles.small_only"]),
    Case("dense4-tiles", _dense4, 8, ["handover.knob", "tiles.order_sort", "tiles.small_only"], env={"BWTS_DENSE": "tiles"}),
    Case("drain-tiles", _drain, 8, ["handover.knob", "tiles.big_groups", "tiles.ends_empty"], env={"BWTS_DENSE": "tiles"}),
    Case("many-factors-twice-tiles", lambda: many_factors_twice(250, 300, 10), 4, ["tiles.stable_rest"], env={"BWTS_DENSE": "tiles"}),
    Case("drain-nomem", _drain, 8, ["handover.no_room_biglist", "tiles.big_groups"], env={"BWTS_BIGLIST_NOMEM": "1"}),
    Case("dense4-wide-keys", _dense4, 8, ["round0.wide"], env={"BWTS_RX_PACK": "0"}),
    Case("dense4-gather", _dense4, 8, ["round0.flags_rank"], env={"BWTS_EMIT": "gather"}),
    Case("recut", _recut, 8, ["chunks.recut_smaller", "chunks.appends_after_recut"], env=CHUNK_TARGET_64),
    Case("recut-drain", _recut_drain, 8, ["chunks.recut_smaller", "chunks.appends_after_recut", "chunks.outgrows_first_cut"], env=CHUNK_TARGET_64),
    Case("suffix-recut", _recut, 8, ["suffix.chunks_biglist", "chunks.recut_smaller", "chunks.appends_after_recut"], sort="suffix", env=CHUNK_TARGET_64),
    Case("general-recut", _recut, 8, ["general.chunks", "chunks.recut_smaller", "chunks.appends_after_recut"], sort="general", env=CHUNK_TARGET_64),
    Case("suffix-sparse", lambda: pasted(1 << 20, 4, 5, [(40, 200)]), 13, ["suffix.sparse"], sort="suffix"),
    Case("suffix-chunks", _drain, 8, ["suffix.chunks_biglist"], sort="suffix"),
    Case("suffix-tiles", lambda: np.concatenate([noise(1 << 18, 200, 13), twice(noise(1 << 13, 200, 14))]), 4, ["suffix.tiles"], sort="suffix"),
    Case("general-sparse", lambda: pasted(1 << 20, 4, 5, [(40, 200)]), 13, ["general.sparse"], sort="general"),
    Case("general-chunks", _drain, 8, ["general.chunks"], sort="general"),
    Case("general-tiles", lambda: np.concatenate([noise(1 << 18, 200, 13), twice(noise(1 << 13, 200, 14))]), 4, ["general.tiles"], sort="general"),
]

# The coverage list, written out: the two "every path" tests hold against it, whatever the cases' tags say.
COVERAGE = [
    "round0.wide", "round0.split32", "round0.split40", "round0.flags_carry", "round0.flags_rank", "round0.nothing_tied",
    "sparse.no_probe", "sparse.probe_small_only", "sparse.probe_compacted", "sparse.whole", "sparse.skip_next", "sparse.directory",
    "sparse.no_directory", "sparse.ends_empty", "sparse.ends_stable",
    "early_ranks.on", "early_ranks.off",
    "chunks.fsl", "chunks.general", "chunks.small_only", "chunks.biglist_leaves_at_once", "chunks.biglist_drains",
    "chunks.biglist_at_stable_end", "chunks.wide", "chunks.stable_rest", "chunks.ends_empty", "chunks.two_rounds_per_trip",
    "chunks.compaction_done", "chunks.recut_smaller", "chunks.appends_after_recut", "chunks.outgrows_first_cut",
    "handover.short_list", "handover.knob", "handover.no_room_biglist",
    "tiles.no_order_sort", "tiles.order_sort", "tiles.big_groups", "tiles.small_only", "tiles.stable_rest", "tiles.ends_empty",
    "suffix.sparse", "suffix.chunks_biglist", "suffix.tiles", "general.sparse", "general.chunks", "general.tiles",
]
assert not {t for c in CASES for t in c.tags} - set(COVERAGE), "a case names a path the list does not have"
NOT_REACHABLE = []
DEFAULT_KEY_CASES = [c for c in CASES if c.sort == "cyclic" and not c.env]       # these run once more with no key knob


def tag_holds(tag, rep):
    """Does the report of one sort (engine's or the model's prediction, same field names) show the path `tag` names?"""
    fam, name = tag.split(".")
    rounds, ch = rep.get("round", []), rep.get("chunks", {})
    if fam == "round0":
        return {"wide": rep.get("keys") == "wide", "split32": rep.get("keys") == "split32", "split40": rep.get("keys") == "split40",
                "flags_carry": rep["flags_outside_rank"], "flags_rank": not rep["flags_outside_rank"], "nothing_tied": rep["tied0"] == 0}[name]
    if fam == "early_ranks":
        return rep["rank_early"] if name == "on" else (not rep["rank_early"] and rep["n"] == (1 << 22) - 1 and rep["tied0"] > rep["n"] // 32)
    if fam in ("suffix", "general"):
        want = {"sparse": "sparse", "chunks_biglist": "chunks", "chunks": "chunks", "tiles": "tiles"}[name]
        return (not rep["cyclic"]) and rep["form"] == want and (name != "chunks_biglist" or ch["m_stay"] > 0)
    if fam == "handover":
        return rep["form"] == "tiles" and rep["no_chunks"] == name
    if fam != rep["form"]:
        return False
    if fam == "sparse":
        return {"no_probe": any(r["probe"] == "short_list" for r in rounds),
                "probe_small_only": any(r["probe"] == "ran" and r["m_big"] == 0 for r in rounds),
                "probe_compacted": any(r["probe"] == "ran" and r["m_big"] > 0 and not r["whole"] for r in rounds),
                "whole": any(r["probe"] == "ran" and r["whole"] for r in rounds),
                "skip_next": any(a["skip_next"] and b["probe"] == "skipped" for a, b in zip(rounds, rounds[1:])),
                "directory": rep.get("directory", 8) >= 8, "no_directory": rep.get("directory", 0) == 0,
                "ends_empty": rep["end"] == "empty", "ends_stable": rep["end"] == "stable"}[name]
    if fam == "chunks":
        # rounds that ran behind a re-cut to a smaller size (the nominal sizes stand beside the dicts that older tests compare whole)
        smaller = [i for i, S in enumerate(rep["chunk_round_S"]) if S < ch["S"]]
        first = -(-ch["a_small"] // ch["S"]) + -(-ch["m_exit"] // ch["S"])          # chunks of the first cut and the first split
        return {"recut_smaller": ch["compactions"] > 0 and 0 < rep["chunk_S_recut"] < ch["S"] and len(smaller) > 0,
                "appends_after_recut": any(rounds[i]["big_leaves"] > 0 for i in smaller),
                # (cuts before round i: the first cut, the first split, one append per earlier round at most, the re-cuts)
                "outgrows_first_cut": any(rounds[i]["nchunks"] > first + 2 + i + ch["compactions"] for i in smaller),
                "fsl": ch["fsl"], "general": not ch["fsl"], "small_only": ch["big0"] == 0,
                "biglist_leaves_at_once": ch["big0"] > 0 and ch["m_stay"] == 0 and ch["m_exit"] == ch["big0"],
                "biglist_drains": ch["m_stay"] > 0 and sum(1 for r in rounds if r["big_leaves"] > 0) >= 2,
                "biglist_at_stable_end": rep["end"] == "stable" and rep["rest_big"] > 0,
                "wide": ch["wide_possible"], "stable_rest": rep["end"] == "stable" and rep["rest_chunks"] > 0,
                "ends_empty": rep["end"] == "empty", "two_rounds_per_trip": ch["enqueued_behind_last"],
                "compaction_done": ch["compactions"] > 0}[name]
    if fam == "tiles":
        return {"no_order_sort": not rep["order_sort"], "order_sort": rep["order_sort"],
                "big_groups": any(r["m_big"] > 0 for r in rounds), "small_only": all(r["m_big"] == 0 for r in rounds),
                "stable_rest": rep["end"] == "stable" and rep["rest_tiles"] > 0, "ends_empty": rep["end"] == "empty"}[name]
    raise KeyError(tag)
