"""GPU suite of range reads of a packed frame (include/bwts_pack.h, "Ranges"): the device's frames of all three versions read through
ranges against the CPU model (tests/pack_range_model.py), the paths by name, what a range read does and does not notice of a damaged
frame, the refusals (each given by the model with the same code first), the committed fixtures, the host form, the memory the call
keeps, and the CLI."""
import ctypes

import numpy as np
import pytest

import pack_range_model as R
import pack_v3_model as P
from test_pack_gpu import _run, _u8
from test_pack_range_model import (B0, BIG, KINDS, N6, SHAPES, bad_range_cases, code_of, damage_cases_of, frame_input, frame_refusal,
                                   golden_frames, model_frame)
from test_pack_v3_model import malformed_cases

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = R.E_ARG, R.E_RANGE, R.E_FORMAT, R.E_SPACE, R.E_CHECKSUM
CANARY = 0xC7
ROOM = 1 << 16


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame; c: output, with room for canaries around it"""
    a, b, c = ctx.alloc(ROOM), ctx.alloc(pkg.pack_bound(ROOM, 4096, version=2) + 64), ctx.alloc(2 * ROOM)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def device_frame(pkg, ctx, bufs, x, block_bytes, version, width):
    """The frame pack_device makes of x, left in b; its bytes."""
    a, b, _ = bufs
    a.upload(_u8(x))
    kw = {"planes": width} if version == 3 else {"version": version}
    size = ctx.pack_device(a, len(x), block_bytes, b, pkg.pack_bound(len(x), block_bytes, **kw), **kw)
    return b.download(size).tobytes()


def read_ranges(ctx, bufs, size, rs, off=0, cap=None):
    """unpack_ranges_device of the frame in b into c + 64 + off: the ranges' bytes one behind the other; the canaries around them must stay."""
    _, b, c = bufs
    total = sum(nb for _, nb in rs)
    c.upload(np.full(total + 192, CANARY, dtype=np.uint8))
    got = ctx.unpack_ranges_device(b, size, rs, c.ptr + 64 + off, total if cap is None else cap)
    assert got == total
    out = c.download(total + 192)
    assert (out[:64 + off] == CANARY).all() and (out[64 + off + total:] == CANARY).all(), "written outside out_bytes"
    return out[64 + off:64 + off + total].tobytes()


def rc_of(pkg, ctx, bufs, size, rs, cap, d_in=None, d_out=None):
    _, b, c = bufs
    arr = np.ascontiguousarray(rs, dtype=np.uint64).reshape(-1, 2)
    got = ctypes.c_uint64(0)
    return pkg.lib().bwts_unpack_ranges_device(ctx._h, b.ptr if d_in is None else d_in, size, arr.ctypes.data if arr.size else None, len(arr),
                                               c.ptr if d_out is None else d_out, cap, ctypes.byref(got))


# -- device frames against the model, and the paths by name ------------------------------------------------------------------
@pytest.mark.parametrize("version,width", KINDS)
def test_device_frames_against_the_model(pkg, ctx, bufs, version, width):
    for n, B in SHAPES:
        x = frame_input(version, n)
        f = device_frame(pkg, ctx, bufs, x, B, version, width)
        assert f == model_frame(version, width, n, B)[1]                # (the device's frame is the model's, byte for byte)
        for name, rs in R.range_sets(n, B or n):
            want = b"".join(R.unpack_ranges(f, rs))
            assert want == b"".join(x[o:o + nb] for o, nb in rs)
            for off in (0, 1, 7):
                assert read_ranges(ctx, bufs, len(f), rs, off) == want, (version, width, n, name, off)
            p, rep = R.plan(f, rs), ctx.debug_unpack_ranges_report()
            assert (rep["blocks"], rep["runs"], rep["covered_bytes"], rep["pieces"]) == (p["blocks"], len(p["runs"]), p["covered_bytes"], len(rs)), name
            assert rep["stream_bytes"] == p["stream_bytes"] and rep["gathered"] == (len(p["runs"]) > 1) and rep["single"] == (p["blocks"] == 1), name
            stages = ["gather"] * rep["gathered"] + ["decode"] + ["zrl"] * (version > 1) + ["mtf", "inverse"] + ["join"] * (version == 3) + ["crc", "cut"]
            assert rep["stages"] == stages, name
            assert ctx.timings().n == p["covered_bytes"]


def test_paths_by_name(pkg, ctx, bufs):
    x = frame_input(2, N6)
    f = device_frame(pkg, ctx, bufs, x, B0, 2, 0)
    sets = dict(R.range_sets(N6, B0))
    at = R.plan(f, [(0, 1)])["stream_at"]
    # one covered block of several: the single-input stages, no gather
    read_ranges(ctx, bufs, len(f), sets["begins at a seam"])
    rep = ctx.debug_unpack_ranges_report()
    assert rep["single"] and not rep["gathered"] and (rep["blocks"], rep["runs"], rep["covered_bytes"]) == (1, 1, B0)
    assert rep["stream_bytes"] == at[3] - at[2]
    # one run of two blocks: the segment stages, the streams read where they lie
    read_ranges(ctx, bufs, len(f), sets["straddles a seam by a byte each side"])
    rep = ctx.debug_unpack_ranges_report()
    assert not rep["single"] and not rep["gathered"] and (rep["blocks"], rep["runs"], rep["covered_bytes"]) == (2, 1, 2 * B0)
    # three runs: the gather ran over exactly the three runs' streams
    read_ranges(ctx, bufs, len(f), sets["three runs"])
    rep = ctx.debug_unpack_ranges_report()
    assert rep["gathered"] and "gather" in rep["stages"] and (rep["blocks"], rep["runs"], rep["covered_bytes"]) == (4, 3, 2 * B0 + B0 + 3)
    assert rep["stream_bytes"] == (at[1] - at[0]) + (at[3] - at[2]) + (at[6] - at[4])
    # B = n: any range covers the one block
    g = device_frame(pkg, ctx, bufs, x[:4097], 0, 2, 0)
    assert read_ranges(ctx, bufs, len(g), [(4096, 1)]) == x[4096:4097]
    rep = ctx.debug_unpack_ranges_report()
    assert rep["single"] and not rep["gathered"] and (rep["blocks"], rep["covered_bytes"]) == (1, 4097)


# -- damage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version,width", KINDS)
def test_damage_is_seen_where_a_range_reads(pkg, ctx, bufs, version, width):
    _, b, c = bufs
    x = frame_input(version, N6)
    f = device_frame(pkg, ctx, bufs, x, B0, version, width)
    got = ctypes.c_uint64(0)
    for name, bad, rs, full, ranged in damage_cases_of(version, x, f)[1]:
        assert code_of(R.unpack_ranges, bad, rs) == ranged, name          # the model first
        b.upload(_u8(bad))
        assert pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(bad), c.ptr, len(x), ctypes.byref(got)) == full != 0, name
        if ranged:
            total = sum(nb for _, nb in rs)
            c.upload(np.full(total + 64, CANARY, dtype=np.uint8))
            assert rc_of(pkg, ctx, bufs, len(bad), rs, total) == ranged, name
            assert (c.download(total + 64) == CANARY).all(), name + ": a failed call wrote to d_out"
        else:
            assert read_ranges(ctx, bufs, len(bad), rs) == b"".join(x[o:o + nb] for o, nb in rs), name


# -- refusals -----------------------------------------------------------------------------------------------------------------
def test_malformed_frames_give_their_codes(pkg, ctx, bufs):
    _, b, c = bufs
    x, f, cases = malformed_cases()
    for name, bad, code in cases:
        n = len(x)
        head = frame_refusal(bad)
        if not head:
            n = int(np.frombuffer(bad[8:16], dtype="<u8")[0])
        rs = [(0, n)]
        assert code_of(R.unpack_ranges, bad, rs) == code, name           # the model first
        padded = bad + bytes(-len(bad) % 16 + 16)
        b.upload(_u8(padded))
        c.upload(np.full(n + 64, CANARY, dtype=np.uint8))
        assert rc_of(pkg, ctx, bufs, len(bad), rs, n) == code, name
        assert (c.download(n + 64) == CANARY).all(), name
        if head:
            # the frame's refusal comes before any range's
            for hostile in ([], [(0, 0)], [(BIG, 2)]):
                assert rc_of(pkg, ctx, bufs, len(bad), hostile, 0) == code, (name, hostile)
    b.upload(_u8(f))
    assert read_ranges(ctx, bufs, len(f), [(B0 - 1, 2)]) == x[B0 - 1:B0 + 1]      # and the context still works


def test_argument_errors(pkg, ctx, bufs):
    a, b, c = bufs
    L = pkg.lib()
    x = frame_input(2, N6)
    f = device_frame(pkg, ctx, bufs, x, B0, 2, 0)
    size, n = len(f), len(x)
    c.upload(np.full(4096, CANARY, dtype=np.uint8))
    for name, rs, cap, code in bad_range_cases(n):
        assert rc_of(pkg, ctx, bufs, size, rs, ROOM if cap is None else cap) == code, name
    many = np.zeros((1 << 20) + 1, dtype=[("o", "<u8"), ("b", "<u8")])
    many["b"] = 1
    got = ctypes.c_uint64(0)
    assert L.bwts_unpack_ranges_device(ctx._h, b.ptr, size, many.ctypes.data, len(many), c.ptr, 1 << 30, ctypes.byref(got)) == E_RANGE
    # out_cap one short: BWTS_E_SPACE and d_out untouched
    assert rc_of(pkg, ctx, bufs, size, [(0, 100), (B0, 100)], 199) == E_SPACE
    one = np.array([[0, 1]], dtype=np.uint64)
    assert L.bwts_unpack_ranges_device(None, b.ptr, size, one.ctypes.data, 1, c.ptr, 1, ctypes.byref(got)) == E_ARG
    assert L.bwts_unpack_ranges_device(ctx._h, None, size, one.ctypes.data, 1, c.ptr, 1, ctypes.byref(got)) == E_ARG
    assert L.bwts_unpack_ranges_device(ctx._h, b.ptr, size, one.ctypes.data, 1, None, 1, ctypes.byref(got)) == E_ARG
    assert L.bwts_unpack_ranges_device(ctx._h, b.ptr, size, one.ctypes.data, 1, c.ptr, 1, None) == E_ARG
    assert L.bwts_unpack_ranges_device(ctx._h, b.ptr, 0, one.ctypes.data, 1, c.ptr, 1, ctypes.byref(got)) == E_ARG
    assert L.bwts_unpack_ranges_device(ctx._h, b.ptr, size, None, 1, c.ptr, 1, ctypes.byref(got)) == E_ARG
    assert rc_of(pkg, ctx, bufs, size, [(0, 1)], 1, d_in=b.ptr + 8) == E_ARG                    # a misaligned d_in
    assert rc_of(pkg, ctx, bufs, size, [(0, 1)], 1, d_out=b.ptr + 16) == E_ARG                  # d_out inside the frame
    assert rc_of(pkg, ctx, bufs, size, [(0, 1)], 64, d_out=b.ptr - 32) == E_ARG                 # d_out's room reaches into it
    assert rc_of(pkg, ctx, bufs, size - 16, [(0, 1)], 1) == E_FORMAT                            # the frame must end at in_bytes
    assert (c.download(4096) == CANARY).all(), "a refused call wrote to d_out"
    assert read_ranges(ctx, bufs, size, [(0, 100), (B0, 100)], cap=200) == x[:100] + x[B0:B0 + 100]


# -- the committed fixtures ------------------------------------------------------------------------------------------------------
def test_golden_frames(pkg, ctx, bufs):
    _, b, _ = bufs
    for name, g in golden_frames():
        n = P.check(g)[1]
        rs = [(n // 3, n // 3 + 1)]
        want = b"".join(R.unpack_ranges(g, rs))
        assert want == P.unpack(g)[n // 3:n // 3 + n // 3 + 1], name
        b.upload(_u8(g))
        assert read_ranges(ctx, bufs, len(g), rs, off=3) == want, name


# -- the host form ---------------------------------------------------------------------------------------------------------------
def test_host_form(pkg, ctx, bufs):
    for version, width in ((1, 0), (3, 4)):
        x = frame_input(version, N6)
        f = device_frame(pkg, ctx, bufs, x, B0, version, width)
        for name, rs in R.range_sets(N6, B0):
            got = ctx.unpack_ranges(f, rs)
            assert [g.tobytes() for g in got] == [x[o:o + nb] for o, nb in rs], (version, name)
            assert b"".join(g.tobytes() for g in got) == read_ranges(ctx, bufs, len(f), rs), name
        assert ctx.unpack_range(f, B0 - 3, 9).tobytes() == x[B0 - 3:B0 + 6]
        rep = ctx.debug_unpack_ranges_report()
        assert not rep["gathered"] and rep["blocks"] == 2                   # the streams arrive back to back: no gather
        ctx.unpack_ranges(f, dict(R.range_sets(N6, B0))["three runs"])
        assert not ctx.debug_unpack_ranges_report()["gathered"] and ctx.debug_unpack_ranges_report()["runs"] == 3
        # after a failure `out` is as it was
        cases = damage_cases_of(version, x, f)[1]
        out = np.full(64, CANARY, dtype=np.uint8)
        got = ctypes.c_uint64(77)
        for name, bad, rs, full, ranged in cases:
            arr = np.ascontiguousarray(rs, dtype=np.uint64)
            src = _u8(bad)
            rc = pkg.lib().bwts_unpack_ranges(ctx._h, src.ctypes.data, src.size, arr.ctypes.data, len(arr), out.ctypes.data, 64, ctypes.byref(got))
            assert rc == ranged, name
            if rc:
                assert (out == CANARY).all() and got.value == 77, name
            else:
                total = sum(nb for _, nb in rs)
                assert out[:total].tobytes() == b"".join(x[o:o + nb] for o, nb in rs) and (out[total:] == CANARY).all() and got.value == total
                out[:] = CANARY
                got.value = 77
        assert E_CHECKSUM in [c[4] for c in cases]
    # the refusals of the host form, in the device form's order
    x, f, cases = malformed_cases()
    out = np.zeros(len(x), dtype=np.uint8)
    for name, bad, code in cases:
        if frame_refusal(bad):
            for rs in ([(0, 1)], []):
                with pytest.raises(pkg.BwtsError) as e:
                    ctx.unpack_ranges(bad, rs)
                assert e.value.code == code, name
    for name, rs, cap, code in bad_range_cases(len(x)):
        arr = np.ascontiguousarray(rs, dtype=np.uint64).reshape(-1, 2)
        src = _u8(f)
        rc = pkg.lib().bwts_unpack_ranges(ctx._h, src.ctypes.data, src.size, arr.ctypes.data if arr.size else None, len(arr), out.ctypes.data,
                                          out.size if cap is None else cap, ctypes.byref(got))
        assert rc == code, name


# -- memory ------------------------------------------------------------------------------------------------------------------------
def test_memory_is_the_covered_bytes(pkg):
    """A frame of 64 blocks of 64 KiB: a range inside one block keeps two blocks of one block's bytes, the full unpack one of n."""
    B, n = 1 << 16, 64 << 16
    x = np.resize(np.frombuffer(frame_input(2, 1 << 16), dtype=np.uint8), n)
    with pkg.Context(0) as one, pkg.Context(0) as two:
        a, b, c = one.alloc(n), one.alloc(pkg.pack_bound(n, B, version=2)), one.alloc(n)
        a.upload(x)
        size = one.pack_device(a, n, B, b, b.nbytes, version=2)
        one.release_memory()
        one.crc32_device(a, 16)
        floor = one.timings().device_bytes                      # what a context keeps for the smallest of calls
        assert floor <= 2 << 20
        assert one.unpack_ranges_device(b, size, [(10 * B + 5, 1000)], c, 1000) == 1000
        ranged = one.timings().device_bytes
        assert np.array_equal(c.download(1000), x[10 * B + 5:10 * B + 1005])
        assert one.debug_unpack_ranges_report()["covered_bytes"] == B
        a2, b2, c2 = two.alloc(16), two.alloc(size), two.alloc(n)
        b2.upload(b.download(size))
        assert two.unpack_device(b2, size, c2, n) == n
        full = two.timings().device_bytes
        print("device_bytes: range read %d, full unpack %d" % (ranged, full))
        assert ranged < full and full >= n
        # released, both are back where the first stood after its release: the arena of the smallest call and the segment table
        for ctx, buf in ((one, a), (two, a2)):
            ctx.release_memory()
            ctx.crc32_device(buf, 16)
            assert ctx.timings().device_bytes == floor
        for d in (a, b, c, a2, b2, c2):
            d.free()


# -- the CLI, each run as a fresh child process ---------------------------------------------------------------------------------------
def test_cli_ranges(tmp_path):
    data = frame_input(2, 3 * 4096 + 77)
    src, packed, back = tmp_path / "in.bin", tmp_path / "in.bwz", tmp_path / "out.bin"
    src.write_bytes(data)
    r = _run("bwts_pack", "-b", 4, "-z", src, packed)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    r = _run("bwts_unpack", "-r", "4090:20", "-r", "0:5", packed, back)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert back.read_bytes() == data[4090:4110] + data[:5]
    r = _run("bwts_unpack", "-r", "%d:1" % (len(data) - 1), packed)            # standard output when no output is named
    assert r.returncode == 0 and r.stdout == data[-1:]
    # two frames, one behind the other: offsets count in the whole unpacked file, and a range may cross from one into the next
    both = tmp_path / "both.bwz"
    both.write_bytes(packed.read_bytes() * 2)
    r = _run("bwts_unpack", "-r", "%d:10" % (len(data) - 4), "-r", "%d:3" % (2 * len(data) - 3), both, back)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert back.read_bytes() == data[-4:] + data[:6] + data[-3:]
    # a range beyond the file: a message that names it, and no output file
    gone = tmp_path / "none.bin"
    r = _run("bwts_unpack", "-r", "0:5", "-r", "%d:2" % (len(data) - 1), packed, gone)
    assert r.returncode == 1 and ("%d:2" % (len(data) - 1)).encode() in r.stderr and not gone.exists()
    for args in (["-r"], ["-r", "5"], ["-r", "5:", packed], ["-r", "a:1", packed], ["-r", "1:1"]):
        r = _run("bwts_unpack", *args)
        assert r.returncode == 1 and r.stderr.strip() and not r.stdout, args
    # without -r nothing changes
    r = _run("bwts_unpack", packed, back)
    assert r.returncode == 0 and back.read_bytes() == data
