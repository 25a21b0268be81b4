"""GPU suite (-m gpu): every layout of the round-0 keys, pinned exactly.

A wrong key never shows in a transform: a key builder that drops a bit, puts a code word wrongly across a word seam or builds a
coarser key at a factor's end only leaves more positions tied, and the later rounds repair the order.  So every cell here compares
the transform with the oracle AND holds the engine's own report (Context.debug_forward_report) against a model that builds every
position's key from the code table alone (tests/key_model.py; fixed-width keys: tests/forward_model.py): the tied count after round 0
is exact, and with it, for the sparse and chunk forms, the tied count of every later round.  tests/test_key_plan.py shows on the CPU
that keys which lose one bit move that count on each input.

Every cell makes a fresh context under BWTS_TEST_KNOBS=1 BWTS_POISON=1 and its own knobs, and FIRST asserts that the report shows the
layout the cell is named for (bits, msym, key_bits, varlen, hstep, keys): no cell can pass on another layout.

  layout                                   pinned by
  fixed, every code width 1..8 bits        test_fixed_grid[w*]          key widths by the maximum and by the heuristic's own pick
  fixed, every key width 8..64 of 1 bit    test_fixed_grid[s2-*]        the seams 16/17, 32/33, 40/41 between wide / split32 / split40 / wide
  fixed, 3-bit codes                       test_fixed_grid[s5-*]        widths that are no multiple of 8
  fixed, below the packed passes           test_fixed_grid[*-n65535]    always wide
  suffix form, the pad costs a bit         test_suffix_grid[s4/s8/s16]
  suffix form, 9-bit codes and pad_add     test_suffix_grid[s256-*]
  variable, the rules' own pick            test_varlen_own_pick         key_bits, hstep against debug_key_plan; sparse and chunk rounds
  variable, every key width                test_varlen_key_bits         lmax, 16 .. 64: every pass count, both split forms, wide
  variable, word seams of the bit stream   test_word_seams
  variable, wrap-around patches            test_wraparound_patches      factors below, at and above the 64-position patch span
  variable, hstep is tight                 test_hstep_is_tight          direct form, and the sparse rounds' variable-length rank search
  variable, the sampled width              test_sampled_width           n = 2^22"""
import json

import numpy as np
import pytest

import forward_cases as FC
import forward_model as M
import key_cases as KC
import key_model as KM
import oracle_lib as O
from test_direct_ties import fresh_context
from test_forward_paths import check_exact, chunk_plan

pytestmark = pytest.mark.gpu

N_SMALL, N_BIG, N_UNPACKED = 65536 + 3, (1 << 17) + 5, 65535


def keys_name(key_bits, n, carry=True):
    """How round 0 keeps keys of this width: split while the packed passes take them (n >= 65536, 17 .. 40 bits), else one u64 each."""
    if not carry or n < 65536 or key_bits <= 16 or key_bits >= 41:
        return "wide"
    return "split32" if key_bits <= 32 else "split40"


def layout_of(rep):
    return {f: rep[f] for f in ("bits", "msym", "key_bits", "varlen", "hstep", "keys")}


_cache = {}


def cached(key, make):
    """One input's oracle results and models, kept while consecutive cells use it."""
    if _cache.get("key") != key:
        _cache.clear()
        _cache.update(key=key, **make())
    return _cache


def run_forward(pkg, x, env):
    with fresh_context(pkg, env) as ctx:
        got = ctx.forward(x)
        t, reps = ctx.timings(), ctx.debug_forward_report()
        back = ctx.inverse(got)
    print(json.dumps(reps))
    return got, back, t, reps


# ---- 1. fixed-width keys -------------------------------------------------------------------------------------------------------------
def fixed_cells():
    cells = []
    for n in (N_SMALL, N_BIG, N_UNPACKED):
        for sigma in (2, 3, 5, 9, 17, 33, 65, 129):
            cells += [("w%d-max-n%d" % (sigma, n), sigma, "0", n), ("w%d-own-n%d" % (sigma, n), sigma, None, n)]
        cells += [("s2-m%d-n%d" % (m, n), 2, str(m), n) for m in (8, 16, 17, 24, 25, 32, 33, 40, 41, 48, 56, 57, 64)]
        cells += [("s5-m%d-n%d" % (m, n), 5, str(m), n) for m in (5, 6, 10, 11, 13, 14, 21)]
    return cells


def noise_input(sigma, n, cyclic):
    def make():
        x = FC.noise(n, sigma, 1000 + sigma)
        d = dict(x=x, mod=M.Model(x, cyclic=cyclic))
        d["want"] = O.forward(x) if cyclic else O.suffix_array(x).astype(np.int64)
        return d
    return cached(("noise", sigma, n, cyclic), make)


@pytest.mark.parametrize("name,sigma,knob,n", fixed_cells(), ids=[c[0] for c in fixed_cells()])
def test_fixed_grid(pkg, name, sigma, knob, n):
    pre = noise_input(sigma, n, True)
    x, mod = pre["x"], pre["mod"]
    bits = (sigma - 1).bit_length()
    own = pkg.debug_key_plan(KC.byte_hist(x), varlen=0)["msym"]
    m = own if knob is None else 64 // bits if knob == "0" else int(knob)
    env = {"BWTS_VARLEN": "0"}
    if knob is not None:
        env["BWTS_KEY_SYMBOLS"] = knob
    got, back, t, reps = run_forward(pkg, x, env)
    assert len(reps) in (1, 2) and reps[-1]["cyclic"], reps
    rep = reps[-1]
    assert layout_of(rep) == {"bits": bits, "msym": m, "key_bits": bits * m, "varlen": False, "hstep": m, "keys": keys_name(bits * m, n)}, layout_of(rep)
    assert np.array_equal(got, pre["want"]) and np.array_equal(back, x)
    check_exact(rep, M.predict(mod, m, chunk_plan(pkg)), t)


def suffix_cells():
    cells = []
    for n in (N_SMALL, N_BIG):
        for sigma in (4, 8, 16):
            cells += [("s%d-max-n%d" % (sigma, n), sigma, "0", n), ("s%d-own-n%d" % (sigma, n), sigma, None, n)]
        cells += [("s256-m%d-n%d" % (m, n), 256, str(m), n) for m in (1, 2, 4, 7)]
    return cells


@pytest.mark.parametrize("name,sigma,knob,n", suffix_cells(), ids=[c[0] for c in suffix_cells()])
def test_suffix_grid(pkg, name, sigma, knob, n):
    """The suffix form keeps code 0 for "past the end": 4, 8 and 16 symbols take one bit more than the cyclic form's codes, and 256
    symbols take 9-bit codes whose table holds 0 .. 255 (the kernels add pad_add = 1)."""
    pre = noise_input(sigma, n, False)
    x, mod = pre["x"], pre["mod"]
    assert np.unique(x).size == sigma
    bits = sigma.bit_length()
    plan = pkg.debug_key_plan(KC.byte_hist(x), reserve_pad=True, varlen=0, key_symbols=knob)
    assert plan["bits"] == bits and plan["pad_add"] == (1 if sigma == 256 else 0)
    m = plan["msym"] if knob is None else 64 // bits if knob == "0" else int(knob)
    env = {"BWTS_VARLEN": "0"}
    if knob is not None:
        env["BWTS_KEY_SYMBOLS"] = knob
    with fresh_context(pkg, env) as ctx:
        sa = ctx.debug_suffix_array(x)
        reps = ctx.debug_forward_report()
    print(json.dumps(reps))
    assert len(reps) == 1 and not reps[0]["cyclic"]
    rep = reps[0]
    assert layout_of(rep) == {"bits": bits, "msym": m, "key_bits": bits * m, "varlen": False, "hstep": m, "keys": "wide"}, layout_of(rep)
    assert np.array_equal(sa.astype(np.int64), pre["want"])
    # the model's keys with the pad code are the classes of the first m symbols (0 past the end)
    keys = KM.fixed_keys(x, None, plan["codes"], bits, m, plan["pad_add"])
    assert KM.tied(keys) == mod.stats(m)["tied"] == rep["tied0"]
    check_exact(rep, M.predict(mod, m, chunk_plan(pkg)))


# ---- 2. variable-length keys ---------------------------------------------------------------------------------------------------------
def varlen_input(pkg, name, build):
    def make():
        x = np.ascontiguousarray(build(), dtype=np.uint8)
        return dict(x=x, want=O.forward(x), starts=O.lyndon_starts(x), hist=KC.byte_hist(x), models={})
    return cached(("varlen", name), make)


def key_model_of(pre, plan):
    """The KeyModel of the input under `plan`'s keys, kept per key width."""
    kb = plan["key_bits"]
    if kb not in pre["models"]:
        keys = KM.keys_of_plan(pre["x"], pre["starts"], plan)
        pre["models"][kb] = (KM.KeyModel(pre["x"], keys, plan["hstep"]), KM.tied(keys))
    return pre["models"][kb]


def check_varlen_cell(pkg, pre, plan, env, exact_rounds=True, lyndon_general=False):
    """One forward under env: the layout `plan` names first, then bytes, then tied0 from the model's keys, then the rounds."""
    x = pre["x"]
    n = x.size
    got, back, t, reps = run_forward(pkg, x, env)
    assert len(reps) in ((2,) if lyndon_general else (1, 2)) and reps[-1]["cyclic"] and not any(r["cyclic"] for r in reps[:-1]), reps
    rep = reps[-1]
    assert plan["varlen"] and plan["hstep"] == plan["msym"] == max(1, plan["key_bits"] // plan["lmax"])
    assert layout_of(rep) == {"bits": plan["bits"], "msym": plan["msym"], "key_bits": plan["key_bits"], "varlen": True, "hstep": plan["hstep"],
                              "keys": keys_name(plan["key_bits"], n)}, (layout_of(rep), plan["key_bits"], plan["lmax"])
    assert t.key_bits == plan["key_bits"] and t.key_symbols == plan["msym"]
    assert np.array_equal(got, pre["want"]), np.flatnonzero(got != pre["want"])[:8]
    assert np.array_equal(back, x)
    mod, tied0 = key_model_of(pre, plan)
    assert rep["tied0"] == tied0 == t.active_after_round0, (rep["tied0"], tied0)
    p = KM.predict_keys(mod, plan, chunk_plan(pkg))
    if rep["form"] != "direct":          # (the direct form is no form of the model's: the caller holds it to its one round)
        assert rep["form"] == p["form"], (rep["form"], p["form"])
        assert [rep["tied0"]] + [r["out"] for r in rep["round"]] == p["round_active"], p["round_active"]
        if exact_rounds and rep["form"] in ("none", "sparse", "chunks"):
            check_exact(rep, p, t)
    return rep


@pytest.mark.parametrize("name", list(KC.VARLEN_INPUTS))
def test_varlen_own_pick(pkg, name):
    """No key knob: geometric draws over 16 and over 40 symbols, the generator's text and real text pick variable-length keys by
    themselves, of the width and first step that debug_key_plan gives for the input's histogram."""
    pre = varlen_input(pkg, name, KC.VARLEN_INPUTS[name])
    plan = pkg.debug_key_plan(pre["hist"])
    assert plan["varlen"]
    rep = check_varlen_cell(pkg, pre, plan, {})
    assert rep["form"] == {"geo16": "sparse", "geo40": "sparse", "text": "chunks", "real": "chunks"}[name]


KEY_BITS = ("lmax", 16, 17, 24, 25, 31, 32, 33, 39, 40, 41, 48, 63, 64)


@pytest.mark.parametrize("kb", KEY_BITS, ids=["kb%s" % k for k in KEY_BITS])
@pytest.mark.parametrize("name", list(KC.VARLEN_INPUTS))
def test_varlen_key_bits(pkg, name, kb):
    """BWTS_VARLEN=1 BWTS_KEY_BITS=kb: 2 .. 8 radix passes, split keys without and with the high byte, wide keys, widths that are no
    multiple of 8, and the narrowest key there is (one longest word: a first step of 1)."""
    pre = varlen_input(pkg, name, KC.VARLEN_INPUTS[name])
    lmax = pkg.debug_key_plan(pre["hist"])["lmax"]
    kb = lmax if kb == "lmax" else kb
    assert kb >= max(8, lmax)
    plan = pkg.debug_key_plan(pre["hist"], varlen=1, key_bits=kb)
    assert plan["key_bits"] == kb
    check_varlen_cell(pkg, pre, plan, {"BWTS_VARLEN": "1", "BWTS_KEY_BITS": str(kb)})


# ---- 3. word seams of the bit stream -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", [None, 64], ids=["own", "kb64"])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65])
def test_word_seams(pkg, k, kb):
    """1-bit and longest words side by side: runs of the 1-bit symbol of 30 .. 34 and 62 .. 66 put code words and key windows at every
    bit offset of a stream word, the longest word stands right before the key builder's tiles end and inside the zero-filled last 64
    positions; sizes end 0, 1, 63, 64 and 65 positions into a tile.  64-bit keys cut their window from three stream words."""
    pre = varlen_input(pkg, "seams%d" % k, lambda: KC.word_seams(k))
    x = pre["x"]
    free = pkg.debug_key_plan(pre["hist"])
    plan = free if kb is None else pkg.debug_key_plan(pre["hist"], varlen=1, key_bits=kb)
    _, common = KC.rarest_and_commonest(x)
    planted = int(x[2047])
    assert free["varlen"] and plan["vlen"][common] == 1 and plan["vlen"][planted] == plan["lmax"] >= 12
    assert all(x[p] == planted for p in (2047, 2048, 8190, 8191, 8192, x.size - 61, x.size - 1)) and x.size == (1 << 16) + 2048 + k
    check_varlen_cell(pkg, pre, plan, {} if kb is None else {"BWTS_VARLEN": "1", "BWTS_KEY_BITS": str(kb)}, exact_rounds=False)


# ---- 4. wrap-around patches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["auto", "general"])
@pytest.mark.parametrize("n", [200000, 3 * 8192 + 5])
def test_wraparound_patches(pkg, n, general):
    """Thousands of Lyndon factors of 2 .. 70 bytes: shorter than, as long as and just longer than the 64 positions in front of a
    factor's end whose keys wrap around.  Every patched key enters the exact tied count; the first radix pass's counts that the
    patches move are pinned with it, because a wrong count breaks the packed sort and the oracle comparison."""
    pre = varlen_input(pkg, "lyndon%d" % n, lambda: KC.descending_lyndon_words_geometric(n, n))
    plan = pkg.debug_key_plan(pre["hist"])
    lens = np.diff(np.append(pre["starts"], n))
    assert plan["varlen"] and lens.size > 1000 and {2, 63, 64, 65} <= set(lens.tolist()) and lens.max() > 65
    rep = check_varlen_cell(pkg, pre, plan, {"BWTS_LYNDON": "general"} if general else {}, exact_rounds=False, lyndon_general=general)
    assert rep["k"] == lens.size


# ---- 5. hstep is tight ---------------------------------------------------------------------------------------------------------------
A = 97                      # key_cases.geo16: the commonest byte
PLANTED_SYM = A + 13        # keeps a longest word after the planting (asserted below)
HSTEP_SPECS = {
    # the runs' starts form one group of 8: the direct form's cap
    "pairs": [(2, [A + 7, A + 8]), (3, [A, A + 1]), (4, [A, A + 1])],
    # twelve copies of the shortest run: a group above the cap
    "big-group": [(2, [A + 7 + i % 8 for i in range(12)]), (3, [A, A + 1]), (4, [A, A + 1])],
}


@pytest.mark.parametrize("name", list(HSTEP_SPECS))
def test_hstep_is_tight(pkg, name):
    """Runs of a longest-word symbol of hstep, hstep + 1 and 2 hstep symbols, each there twice (or twelve times) with different
    symbols behind: the key of a run's start covers the run and at most a few bits of what follows, so the copies are tied after
    round 0 and come apart at the first symbol the key did not cover -- hstep symbols in, or one more.  A first step longer than hstep
    would jump over that symbol.  "pairs": the direct form settles every group; "big-group": a group above its cap sends the list
    to the sparse rounds, whose rank search builds variable-length keys of untied successors."""
    pre = varlen_input(pkg, "hstep-" + name, lambda: KC.planted_runs(HSTEP_SPECS[name], PLANTED_SYM)[0])
    x = pre["x"]
    _, where = KC.planted_runs(HSTEP_SPECS[name], PLANTED_SYM)
    plan = pkg.debug_key_plan(pre["hist"])
    h = plan["hstep"]
    assert plan["varlen"] and plan["vlen"][PLANTED_SYM] == plan["lmax"] and sorted(where) == [h, h + 1, 2 * h]
    mod, tied0 = key_model_of(pre, plan)
    kc, sym = mod.classes(h), M.Model(x)
    for length, starts in where.items():
        assert len(set(kc[starts].tolist())) == 1, "the copies are tied after round 0"
        assert len(set(sym.classes(length + 1)[starts].tolist())) > 1, "and differ right behind the run"
    sizes = np.bincount(kc)
    assert tied0 <= x.size // 32 and (sizes.max() == 8 if name == "pairs" else sizes.max() > 8)
    rep = check_varlen_cell(pkg, pre, plan, {"BWTS_DIRECT_MIN_LOG2": "0"})
    if name == "pairs":
        assert (rep["direct_word"], rep["form"], rep["rounds"], rep["left"]) == (1, "direct", 2, 0), rep
        assert rep["round"] == [{"form": "direct", "h": h, "in": tied0, "out": 0, "splits": 1}]
    else:
        assert (rep["direct_word"], rep["form"]) == (2, "sparse"), rep


# ---- 6. the sampled width ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["geo8", "geo40"])
def test_sampled_width(pkg, name):
    """n = 2^22, a 64 KiB block 64 times: the key sample sees far more equal keys than the i.i.d. model allows and asks for 64 bits.
    The report does not carry the sample, so the cell names the branch of key_plan.h it expects: with words of at most 10 bits the
    engine keeps 40 key bits (a first step of four symbols already), with longer words it takes the sampled 64."""
    def make():
        block = KC.geo8(1 << 16) if name == "geo8" else KC.geo40(1 << 16)
        x = np.tile(block, 64)
        return dict(x=x, want=O.forward(x), hist=KC.byte_hist(x))
    pre = cached(("sampled", name), make)
    x = pre["x"]
    model = pkg.debug_key_plan(pre["hist"])
    sampled = pkg.debug_key_plan(pre["hist"], kb_emp=64, partners_of=np.full(65, 32.0))
    assert model["varlen"] and sampled["varlen"] and model["kb_iid"] < 64
    if name == "geo8":
        assert model["lmax"] <= 10 and sampled["key_bits"] == 40, "the `keep` branch"
    else:
        assert model["lmax"] >= 11 and sampled["key_bits"] == 64 != model["key_bits"], "the sampled width"
    got, back, t, reps = run_forward(pkg, x, {})
    rep = reps[-1]
    assert rep["cyclic"] and layout_of(rep) == {"bits": sampled["bits"], "msym": sampled["msym"], "key_bits": sampled["key_bits"], "varlen": True,
                                                "hstep": sampled["hstep"], "keys": keys_name(sampled["key_bits"], x.size)}, layout_of(rep)
    assert np.array_equal(got, pre["want"]) and np.array_equal(back, x)
