"""GPU suite of the two chains of pack.hip (encode_chain, decode_chain): one table of frames that meets every stage set of both at the
smallest sizes where they differ -- "BWTZ" versions 1, 2 and 3, member frames without and with a split, without and with a filter --
each as one block (the single-input stages) and as several (the segment forms).  Every frame is packed on the device and held byte for
byte against the CPU model, unpacked whole between canaries, read through a range that covers one block and through two separated
runs (which gathers), and, a member frame, read by members.  The whole unpack lands in d_out whatever the number of stages
(3 + zrl + split + delta, every parity here); the range reads report exactly the stages that apply to the blocks they cover."""
import functools

import numpy as np
import pytest

import pack_members_model as MM
import pack_members_v2_model as M2
import pack_model as P1
import pack_v2_model as P2
import pack_v3_model as P3
from members_v2_cases import walk
from test_pack_gpu import _first_diff, _u8
from test_pack_model import fixture_input
from test_pack_v3_model import typed_input

pytestmark = pytest.mark.gpu

CANARY = 0xC7
B = 4096
N_ONE = 4099                            # one block: a tile and three bytes, no multiple of any width above 1
N_SEVERAL = 3 * B + 3                   # four blocks, the last of 3 bytes
LENGTHS = [4096, 1, 4099, 8192]         # members: a member of one byte, one of no multiple of its width
ROOM = 1 << 15

# (name, version, width) and (name, widths of the four members, filters, width and filter of the one member)
BWTZ = [("v1", 1, 0), ("v2", 2, 0), ("v3 w4", 3, 4)]
BWTM = [("widths 1", [1, 1, 1, 1], None, 1, 0),
        ("mixed widths", [1, 2, 4, 8], None, 8, 0),
        ("a filter at width 1", [1, 1, 1, 1], [1, 0, 1, 0], 1, 1),
        ("a filter at width 4, no other member split", [1, 1, 1, 4], [0, 0, 0, 1], 4, 1),
        ("mixed widths and filters", [1, 2, 4, 8], [1, 0, 1, 1], 2, 1)]
FRAMES = [("BWTZ %s, %s" % (k[0], shape), "z", k, shape) for k in BWTZ for shape in ("one block", "several")] + \
         [("BWTM %s, %s" % (k[0], shape), "m", k, shape) for k in BWTM for shape in ("one block", "several")]


@functools.lru_cache(maxsize=None)
def model(i):
    """(x, frame, lengths, widths, filters, zrl) of FRAMES[i] by the CPU models: made once, shared, left unchanged.  lengths, widths
    and filters are per block; widths 1 and filters 0 where the frame has none."""
    _, magic, kind, shape = FRAMES[i]
    if magic == "z":
        _, version, width = kind
        n, block = (N_ONE, 0) if shape == "one block" else (N_SEVERAL, B)
        x = typed_input(n, 77 + n) if version == 3 else fixture_input(n, 77 + n + version)
        f = P1.pack(x, block) if version == 1 else P2.pack(x, block) if version == 2 else P3.pack(x, width, block)
        lengths = [n] if not block else [min(B, n - k * B) for k in range(-(-n // B))]
        return x, f, lengths, [width or 1] * len(lengths), [0] * len(lengths), version > 1
    _, widths, filters, w1, f1 = kind
    lengths, widths, filters = ([N_ONE], [w1], [f1]) if shape == "one block" else (LENGTHS, widths, filters or [0] * 4)
    members = [walk(ln, w, 9 + k) if fl else fixture_input(ln, 300 + k) for k, (ln, w, fl) in enumerate(zip(lengths, widths, filters))]
    f = M2.pack(members, widths, filters) if any(filters) else MM.pack(members, widths)
    return b"".join(members), f, lengths, widths, filters, True


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame; c: output, with room for canaries around it"""
    a, b, c = ctx.alloc(ROOM), ctx.alloc(pkg.pack_members_bound([ROOM // 4] * 4) + 64), ctx.alloc(2 * ROOM)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def between_canaries(c, total, call):
    """call(pointer 64 bytes into c) must write `total` bytes there and nothing around them: those bytes."""
    c.upload(np.full(total + 192, CANARY, dtype=np.uint8))
    assert call(c.ptr + 64) == total
    out = c.download(total + 192)
    assert (out[:64] == CANARY).all() and (out[64 + total:] == CANARY).all(), "written outside the output"
    return out[64:64 + total].tobytes()


def stages_of(pkg, covered, widths, filters, zrl, gathered):
    """The stage list of a range read over the covered blocks, as the report names it."""
    ran = ["gather"] * gathered + ["decode"] + ["zrl"] * zrl + ["mtf", "inverse"] + ["join"] * any(widths[k] != 1 for k in covered) + \
          ["delta"] * any(filters[k] for k in covered) + ["crc", "cut"]
    return [name for name in pkg.RANGES_STAGES.values() if name in ran]


@pytest.mark.parametrize("i", range(len(FRAMES)), ids=[f[0] for f in FRAMES])
def test_frame_through_both_chains(pkg, ctx, bufs, i):
    name, magic, kind, shape = FRAMES[i]
    x, f, lengths, widths, filters, zrl = model(i)
    a, b, c = bufs
    n, count = len(x), len(lengths)
    off = [sum(lengths[:k]) for k in range(count + 1)]
    assert n == (N_ONE if shape == "one block" else N_SEVERAL if magic == "z" else sum(LENGTHS)) and len(f) + 64 <= b.nbytes

    # encode: the device's frame is the model's
    a.upload(_u8(x))
    if magic == "z":
        kw = {"planes": kind[2]} if kind[1] == 3 else {"version": kind[1]}
        block = 0 if shape == "one block" else B
        size = ctx.pack_device(a, n, block, b, pkg.pack_bound(n, block, **kw), **kw)
    else:
        size = ctx.pack_members_device(a, lengths, widths, b, pkg.pack_members_bound(lengths), filters=filters if any(filters) else None)
    y = b.download(size)
    assert size == len(f) and y.tobytes() == f, "pack: %s" % _first_diff(y, _u8(f))

    # decode, all blocks: the last stage lands in d_out, whatever the number of stages
    got = between_canaries(c, n, lambda p: ctx.unpack_device(b, size, p, n))
    assert got == x, "unpack: %s" % _first_diff(_u8(got), _u8(x))
    assert ctx.timings().n == n

    # decode, one covered block (the single-input stages, the stream read where it lies) ...
    k = 1 if magic == "z" and count > 1 else 2 if count > 1 else 0
    reads = [("one block", [(off[k] + 7, min(100, lengths[k] - 7))], [k], False)]
    # ... and two separated runs: the first block, and behind an uncovered one the last two ("BWTZ") or the last one
    if count > 1:
        far = [2, 3] if magic == "z" else [3]
        reads.append(("two runs", [(off[far[0]] + lengths[far[0]] - 10, 12 if len(far) == 2 else 10), (5, 10)], [0] + far, True))
    for what, rs, covered, gathered in reads:
        total = sum(nb for _, nb in rs)
        got = between_canaries(c, total, lambda p: ctx.unpack_ranges_device(b, size, rs, p, total))
        assert got == b"".join(x[o:o + nb] for o, nb in rs), (name, what)
        rep = ctx.debug_unpack_ranges_report()
        assert (rep["blocks"], rep["runs"], rep["covered_bytes"]) == (len(covered), 2 if gathered else 1, sum(lengths[j] for j in covered)), (name, what)
        assert rep["gathered"] == gathered and rep["single"] == (len(covered) == 1), (name, what)
        assert rep["stages"] == stages_of(pkg, covered, widths, filters, zrl, gathered), (name, what, rep["stages"])
        assert ctx.timings().n == rep["covered_bytes"]

    # decode by members: the last and the first, in that order
    if magic == "m":
        idx = [count - 1, 0]
        total = sum(lengths[j] for j in idx)
        got = between_canaries(c, total, lambda p: ctx.unpack_members_device(b, size, idx, p, total))
        assert got == b"".join(x[off[j]:off[j + 1]] for j in idx), name
        rep = ctx.debug_unpack_ranges_report()
        covered = sorted(set(idx))
        assert rep["blocks"] == len(covered) and rep["stages"] == stages_of(pkg, covered, widths, filters, True, count > 2), (name, rep["stages"])
