"""CPU suite of the move-to-front stage: the definition's known answers, the tiled state algebra against the serial loop, the new
header against the library and MTF_EXPORTS, and the tile plan's arithmetic."""
import os
import re

import numpy as np
import pytest

import mtf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs():
    rng = np.random.default_rng(5)
    n = 3000
    uniform = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    zipf = (np.minimum(rng.zipf(1.3, n), 256) - 1).astype(np.uint8).tobytes()
    runs = b"".join(bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 131)) for _ in range(60))
    few = rng.choice(np.array([7, 200, 100], dtype=np.uint8), n).tobytes()
    # a few tiles at the shipped tile size, so that its rows compose: runs, and a few symbols with a late first occurrence
    tiles3 = bytearray(b"".join(bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 131)) for _ in range(400))[:3 * 4096 + 5])
    assert len(tiles3) == 3 * 4096 + 5
    late = bytearray(rng.choice(np.array([7, 200, 9], dtype=np.uint8), 3 * 4096 + 5).tobytes())
    late[2 * 4096 + 100] = 100
    return {"tiles3": bytes(tiles3), "late": bytes(late), "uniform": uniform, "zipf": zipf, "runs": runs, "few": few, "cycle": bytes(range(256)) * 3 + b"\x05",
            "down": bytes(range(255, -1, -1)) * 2, "one": b"\x09", "same": b"\x2a" * 700}


INPUTS = _inputs()


def test_known_answers():
    assert M.forward(bytes([1, 1, 0, 2, 2, 1])) == bytes([1, 0, 1, 2, 0, 2])
    assert M.forward(bytes(range(256)) * 2) == bytes(range(256)) + bytes([255]) * 256
    assert M.inverse(bytes([1, 0, 1, 2, 0, 2])) == bytes([1, 1, 0, 2, 2, 1])
    assert M.forward(b"") == b"" and M.inverse(b"") == b""


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_inverse_undoes_forward_and_forward_undoes_inverse(name):
    x = INPUTS[name]
    assert M.inverse(M.forward(x)) == x
    assert M.forward(M.inverse(x)) == x          # any bytes are ranks of something
    assert M.forward_fast(x) == M.forward(x)
    assert M.inverse_fast(x) == M.inverse(x)


@pytest.mark.parametrize("T", [1, 4, 64, 4096])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_tiled_equals_serial(name, T):
    x = INPUTS[name]
    if T == 1:
        x = x[:400]
    elif T < 4096:
        x = x[:3000]
    assert M.forward_tiled(x, T) == M.forward(x)
    assert M.inverse_tiled(x, T) == M.inverse(x)


@pytest.mark.parametrize("T", [1, 4, 64, 4096])
def test_tiled_equals_serial_with_segments(T):
    rng = np.random.default_rng(11)
    for name in ("uniform", "runs", "few", "tiles3"):
        x = INPUTS[name][:1200 if T == 1 else 3000 if T < 4096 else None]
        lengths, left = [], len(x)
        while left:
            m = int(min(left, rng.integers(1, 3 * max(T, 40))))
            lengths.append(m)
            left -= m
        want_f, want_i = M.segmented(M.forward, x, lengths), M.segmented(M.inverse, x, lengths)
        assert M.forward_tiled(x, T, lengths) == want_f
        assert M.inverse_tiled(x, T, lengths) == want_i
        assert M.segmented(M.inverse, want_f, lengths) == x
    assert M.forward_tiled(INPUTS["few"], T, [len(INPUTS["few"])]) == M.forward(INPUTS["few"])


def test_compose_is_associative_and_carries_unseen_order():
    """The late first occurrence: a symbol no earlier tile has seen keeps its place among the never-seen ones, and d counts the union."""
    a, b, c = M.forward_state(bytes([7, 200, 7])), M.forward_state(bytes([9, 9, 3])), M.forward_state(bytes([100, 7]))
    left = M.forward_compose(M.forward_compose(a, b), c)
    right = M.forward_compose(a, M.forward_compose(b, c))
    assert left == right == M.forward_state(bytes([7, 200, 7, 9, 9, 3, 100, 7]))
    assert left[1] == 5
    pa, pb, pc = (M.inverse_state(t)[1] for t in (bytes([3, 0, 255]), bytes([1, 1, 200]), bytes([0, 9])))
    assert M.inverse_compose(M.inverse_compose(pa, pb), pc) == M.inverse_compose(pa, M.inverse_compose(pb, pc))


def test_header_symbols_exported(pkg):
    L = pkg.lib()
    header = open(os.path.join(ROOT, "include", "bwts_mtf.h")).read()
    declared = sorted(set(re.findall(r"\b(bwts_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations parsed"
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(pkg.MTF_EXPORTS) == declared
    assert not set(pkg.MTF_EXPORTS) & set(pkg.EXPORTS + pkg.TEST_EXPORTS)


def test_null_arguments_rejected_without_a_device(pkg):
    L = pkg.lib()
    for name in ("bwts_mtf_forward", "bwts_mtf_inverse", "bwts_mtf_forward_device", "bwts_mtf_inverse_device"):
        assert getattr(L, name)(None, None, 5, None) == -1
    for name in ("bwts_mtf_forward_segments", "bwts_mtf_inverse_segments", "bwts_mtf_forward_segments_device", "bwts_mtf_inverse_segments_device"):
        assert getattr(L, name)(None, None, None, 1, None) == -1


def test_plan_is_consistent(pkg):
    p1 = pkg.debug_mtf_plan(1)
    T, G = p1["T"], p1["G"]
    assert T >= 64 and G >= 2 and p1["tiles"] == 1 and p1["groups"] == 1
    for n in (1, T, T + 1, G * T, G * T + 1, 2 * G * T + T + 7, 1 << 36):
        p = pkg.debug_mtf_plan(n)
        assert (p["T"], p["G"]) == (T, G)
        assert p["tiles"] == -(-n // T) and p["groups"] == -(-p["tiles"] // G)
    assert pkg.debug_mtf_plan(G * T)["groups"] == 1 and pkg.debug_mtf_plan(G * T + 1)["groups"] == 2
    with pytest.raises(pkg.BwtsError):
        pkg.debug_mtf_plan(0)
