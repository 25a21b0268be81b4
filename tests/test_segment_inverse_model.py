"""CPU suite: the segmented inverse's shared pass as a model (tests/segment_inverse_model.py) against the oracle, and the host-side
plan of bwts_inverse_segments (bwts_debug_segments_plan: no context, no device).  Exact bytes and counts; no tolerance."""
import numpy as np
import pytest

import oracle_lib as O
import segment_cases as C
import segment_inverse_model as SM

EDGE_LENGTHS = (15, 16, 17, 63, 64, 65)         # around the splitter spacing (16) and the slot (64) of g = 4


def _random_set(rng):
    count = int(rng.integers(1, 10))
    lengths = rng.integers(1, 81, count)
    for i in rng.integers(0, count, int(rng.integers(0, 3))):
        lengths[i] = EDGE_LENGTHS[int(rng.integers(len(EDGE_LENGTHS)))]
    sigma = int(rng.integers(1, 5))
    data = rng.integers(0, sigma, int(lengths.sum())).astype(np.uint8) + np.uint8(97)
    return data, lengths.astype(np.uint64)


@pytest.mark.parametrize("seed", range(8))
def test_model_inverse_equals_oracle_on_random_sets(seed):
    rng = np.random.default_rng(1000 + seed)
    seen = set()
    for _ in range(40):
        data, lengths = _random_set(rng)
        seen |= set(int(x) for x in lengths)
        m = SM.SegmentModel(data, lengths)
        assert np.array_equal(m.inverse(), C.expected_inverse(data, lengths)), (data.tolist(), lengths.tolist())
        assert m.cycles == C.expected_factors(C.expected_inverse(data, lengths), lengths)
    assert seen & set(EDGE_LENGTHS)


def test_model_inverse_every_edge_length_in_one_set():
    lengths = np.array(list(EDGE_LENGTHS) + [1, 2, 80, 3], dtype=np.uint64)
    for sigma in (1, 2, 3, 4):
        data = np.random.default_rng(sigma).integers(0, sigma, int(lengths.sum())).astype(np.uint8)
        m = SM.SegmentModel(data, lengths)
        assert np.array_equal(m.inverse(), C.expected_inverse(data, lengths))


@pytest.mark.parametrize("seed", [3, 4])
def test_model_inverse_equals_tiny_table(seed):
    data, lengths = C.tiny_segments(seed, 5000)
    table = C.TinyTable(O.inverse)
    m = SM.SegmentModel(data, lengths)
    assert np.array_equal(m.inverse(), table.apply(data, lengths))
    assert m.cycles == table.count_factors(table.apply(data, lengths), lengths)


def test_model_lf_is_the_per_segment_lf_with_global_indices():
    import inverse_model as M
    data, lengths = _random_set(np.random.default_rng(5))
    off = SM.bounds(lengths)
    LF = SM.segment_lf_map(data, lengths)
    for s in range(len(lengths)):
        a, b = int(off[s]), int(off[s + 1])
        assert np.array_equal(LF[a:b], a + M.lf_map(data[a:b]))


# ---- the plan: host arithmetic ----------------------------------------------------------------------------------------------------

def test_plan_1024_segments_of_1mib_share_one_pass(pkg):
    p = pkg.debug_segments_plan(np.full(1024, 1 << 20, dtype=np.uint64))
    assert p["plan"] == "shared" and p["runs"] == 1 and p["big"] > 1 << 20, p
    assert (p["shared_segments"], p["shared_bytes"]) == (1024, 1 << 30), p
    assert (p["lane_segments"], p["lane_bytes"], p["single_segments"], p["single_bytes"]) == (0, 0, 0, 0), p
    assert p["arena_bytes"] > 8 << 30, p                  # about what a single inverse of the run holds, not 4 n


def test_plan_a_million_3_byte_segments_stay_on_the_lane_walk(pkg):
    p = pkg.debug_segments_plan(np.full(1 << 20, 3, dtype=np.uint64))
    assert p["plan"] == "lane" and p["runs"] == 1, p
    assert (p["lane_segments"], p["lane_bytes"]) == (1 << 20, 3 << 20), p
    assert (p["shared_segments"], p["shared_bytes"], p["single_segments"], p["single_bytes"]) == (0, 0, 0, 0), p
    assert p["arena_bytes"] == 4 * (3 << 20) + (1 << 16), p


def test_plan_one_64mib_segment_among_64k_ones_goes_single(pkg):
    ls = np.full(2049, 1 << 16, dtype=np.uint64)
    ls[1000] = 64 << 20
    p = pkg.debug_segments_plan(ls)
    assert (p["single_segments"], p["single_bytes"]) == (1, 64 << 20), p
    assert 1 << 16 < p["big"] <= 64 << 20, p
    own = "shared" if p["plan"] == "shared" else "lane"
    assert (p[own + "_segments"], p[own + "_bytes"]) == (2048, 2048 << 16), p
    assert p["runs"] == (2 if p["plan"] == "shared" else 1), p


def test_plan_rejects_bad_lengths(pkg):
    for ls in ([], [0], [5, 0, 3], [1 << 32, 1]):
        with pytest.raises(pkg.BwtsError):
            pkg.debug_segments_plan(np.array(ls, dtype=np.uint64))
