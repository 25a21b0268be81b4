"""GPU suite of pack / unpack with frames of version 3 (include/bwts_pack.h): every frame byte for byte against the CPU model
(tests/pack_v3_model.py), the device's frame and the model's frame unpacked on the device back to the input, the capacity contract,
frames of all three versions through the same unpack, the committed fixtures, the malformed version-3 frames (each refused by the
model with the same code first), the host forms, the memory the calls keep, and the CLIs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pack_model as P1
import pack_v2_model as P2
import pack_v3_model as P
import planes_model as S
from test_pack_gpu import PKG_DIR, _first_diff, _run, _u8, content
from test_pack_v3_model import FIXTURES, GOLDEN, malformed_cases, typed_input

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
TOP = (1 << 20) + 5
SHAPES = [(4096, 3 * 4096 + 1), (4097, 40 * 4097 + 9), (65536, TOP)]


def f32_content(n):
    """n bytes of the smooth float32 field of the size tables (the last value cut where n is no multiple of 4)."""
    return np.frombuffer(P.f32_field(-(-n // 4))[:n], dtype=np.uint8)


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame, as large as the bound of the largest input; c: output"""
    a, c = ctx.alloc(TOP + 64), ctx.alloc(TOP + 64)
    b = ctx.alloc(pkg.pack_bound(TOP, 4096, planes=4) + 64)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def _checked(pkg, ctx, bufs, x, w, block_bytes, capacity=True):
    """The checks of one input: device frame == model frame, device unpack of both == x, exact capacity, capacity - 16."""
    x = _u8(x)
    n = x.size
    a, b, c = bufs
    want = _u8(P.pack(x, w, block_bytes))
    a.upload(x)
    size = ctx.pack_device(a, n, block_bytes, b, pkg.pack_bound(n, block_bytes, planes=w), planes=w)
    assert size == want.size, (n, w, block_bytes, size, want.size)
    y = b.download(size)
    assert np.array_equal(y, want), "pack n=%d w=%d B=%d: %s" % (n, w, block_bytes, _first_diff(y, want))
    assert ctx.timings().n == n
    c.upload(np.zeros(n, dtype=np.uint8) if x.any() else np.ones(n, dtype=np.uint8))
    assert ctx.unpack_device(b, size, c, n) == n
    back = c.download(n)
    assert np.array_equal(back, x), "unpack n=%d w=%d B=%d: %s" % (n, w, block_bytes, _first_diff(back, x))
    assert P.unpack(want.tobytes()) == x.tobytes()          # the model's frame, through the model ...
    b.upload(want)                                          # ... and through the device
    c.upload(np.zeros(n, dtype=np.uint8) if x.any() else np.ones(n, dtype=np.uint8))
    assert ctx.unpack_device(b, want.size, c, n + 5) == n
    assert np.array_equal(c.download(n), x)
    assert ctx.timings().n == n
    if capacity:
        mark = np.full(size + 64, 0xA5, dtype=np.uint8)
        b.upload(mark)
        assert ctx.pack_device(a, n, block_bytes, b, size, planes=w) == size                     # exact capacity
        assert np.array_equal(b.download(size + 64), np.concatenate((want, mark[size:])))
        b.upload(mark)
        got = ctypes.c_uint64(0)
        rc = pkg.lib().bwts_pack_planes_device(ctx._h, w, a.ptr, n, block_bytes, b.ptr, size - 16, ctypes.byref(got))
        assert rc == E_SPACE, (n, rc)
        assert np.array_equal(b.download(size + 64), mark), "BWTS_E_SPACE, but something was written"      # the marks, everywhere
    return want


@pytest.mark.parametrize("w", P.WIDTHS)
def test_one_block(pkg, ctx, bufs, w):
    for n in (1, w - 1, w + 1, 4095, 4097, 65537):
        for make in (f32_content, lambda m: content("zipf", m)):
            f = _checked(pkg, ctx, bufs, make(n), w, 0, capacity=n <= 4097)
            assert f[4:8].view("<u4")[0] == 3 and f[16:24].view("<u8")[0] == n and f[44:48].view("<u4")[0] == w


@pytest.mark.parametrize("block,n", SHAPES)
def test_blocks(pkg, ctx, bufs, block, n):
    f = _checked(pkg, ctx, bufs, f32_content(n), 4, block)
    assert f[8:24].view("<u8").tolist() == [n, block]
    nblk = -(-n // block)
    assert (f[32:32 + 32 * nblk].view("<u4")[3::8] == 4).all()            # the width word of every entry
    if n < (1 << 20):
        for name, w in (("text", 2), ("zipf", 8), ("uniform256", 4), ("repeat", 8), ("ab", 2)):
            _checked(pkg, ctx, bufs, content(name, n), w, block, capacity=False)
        # blocks that are stored beside blocks that are coded
        mixed = f32_content(n).copy()
        mixed[block:2 * block] = content("uniform256", block)
        _checked(pkg, ctx, bufs, mixed, 4, block, capacity=False)
    else:
        _checked(pkg, ctx, bufs, content("text", n), 8, block, capacity=False)


def test_the_gain_on_the_device(pkg, ctx, bufs):
    """What test_pack_v3_model asserts of the model, of the device's frames: the 256 KiB float32 field at width 4 under 0.8 of its
    version-2 frame."""
    a, b, c = bufs
    x = f32_content(1 << 18)
    a.upload(x)
    v2 = ctx.pack_device(a, x.size, 0, b, pkg.pack_bound(x.size, 0, version=2), version=2)
    v3 = ctx.pack_device(a, x.size, 0, b, pkg.pack_bound(x.size, 0, planes=4), planes=4)
    print("f32 field: version 2 %d bytes, version 3 at width 4 %d bytes, ratio %.4f" % (v2, v3, v3 / v2))
    assert v3 < 0.8 * v2
    assert ctx.unpack_device(b, v3, c, x.size) == x.size and np.array_equal(c.download(x.size), x)


def test_all_versions_through_the_same_call(pkg, ctx, bufs):
    a, b, c = bufs
    for x, block in ((f32_content(70001), 0), (content("text", 5 * 4096 + 3), 4096)):
        n = x.size
        a.upload(x)
        want = (P1.pack(x, block), P2.pack(x, block), P.pack(x, 4, block))
        for k, kw in enumerate(({"version": 1}, {"version": 2}, {"planes": 4})):
            size = ctx.pack_device(a, n, block, b, pkg.pack_bound(n, block, **kw), **kw)
            assert b.download(size).tobytes() == want[k], kw
            assert b.download(8)[4] == k + 1
            c.upload(np.zeros(n, dtype=np.uint8))
            assert ctx.unpack_device(b, size, c, n) == n and np.array_equal(c.download(n), x), kw
        assert ctx.pack_device(a, n, block, b, pkg.pack_bound(n, block, planes=4), version=3, planes=4) == len(want[2])
    # version 3 is asked for with a width: the _v calls still refuse it, and planes goes with no other version
    got = ctypes.c_uint64(0)
    host = np.zeros(64, dtype=np.uint8)
    assert pkg.lib().bwts_pack_device_v(ctx._h, 3, a.ptr, 5000, 0, b.ptr, 1 << 20, ctypes.byref(got)) == E_ARG
    assert pkg.lib().bwts_pack_v(ctx._h, 3, host.ctypes.data, 16, 0, host.ctypes.data, 64, ctypes.byref(got)) == E_ARG
    for w in (0, 1, 3, 16):
        assert pkg.lib().bwts_pack_planes_device(ctx._h, w, a.ptr, 5000, 0, b.ptr, 1 << 20, ctypes.byref(got)) == E_ARG
        assert pkg.lib().bwts_pack_planes(ctx._h, w, host.ctypes.data, 16, 0, host.ctypes.data, 64, ctypes.byref(got)) == E_ARG
    assert pkg.lib().bwts_pack_planes_device(ctx._h, 4, a.ptr, 5000, 100, b.ptr, 1 << 20, ctypes.byref(got)) == E_ARG
    assert pkg.lib().bwts_pack_planes_device(ctx._h, 4, a.ptr, (1 << 32) + 1, 0, b.ptr, 1 << 20, ctypes.byref(got)) == E_RANGE
    assert pkg.lib().bwts_pack_planes_device(ctx._h, 4, a.ptr, 5000, 0, b.ptr + 8, 1 << 20, ctypes.byref(got)) == E_ARG          # d_out off 16 bytes
    assert pkg.lib().bwts_pack_planes_device(ctx._h, 4, a.ptr, 5000, 0, a.ptr + 4992, 1 << 20, ctypes.byref(got)) == E_ARG       # overlap
    for kw in ({"version": 1, "planes": 4}, {"version": 2, "planes": 4}, {"version": 3}):
        with pytest.raises(pkg.BwtsError):
            ctx.pack_device(a, 5000, 0, b, 1 << 20, **kw)
        with pytest.raises(pkg.BwtsError):
            ctx.pack(host, **kw)


def test_golden_fixtures_unpack_on_the_device(ctx, bufs):
    a, b, c = bufs
    for name, (x, w, B) in FIXTURES.items():
        f = _u8(open(os.path.join(GOLDEN, name), "rb").read())
        b.upload(f)
        c.upload(np.zeros(len(x), dtype=np.uint8))
        assert ctx.unpack_device(b, f.size, c, len(x)) == len(x)
        assert c.download(len(x)).tobytes() == x, name
        a.upload(_u8(x))
        assert ctx.pack_device(a, len(x), B, b, f.size, planes=w) == f.size and np.array_equal(b.download(f.size), f), name


def test_malformed_frames(pkg, ctx, bufs):
    a, b, c = bufs
    x, f, cases = malformed_cases()
    got = ctypes.c_uint64(0)
    for name, bad, code in [("valid", f, 0)] + cases:
        try:
            P.unpack(bad)
            model = 0
        except P.PackError as e:
            model = e.code
        assert model == code, name                           # refused by the model, with this code, first
        b.upload(_u8(bad))
        rc = pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(bad), c.ptr, len(x) + 4096, ctypes.byref(got))
        assert rc == code, "%s: %d, the model says %d" % (name, rc, code)
    # a header n beyond out_cap, and the context still works afterwards
    b.upload(_u8(f))
    assert pkg.lib().bwts_unpack_device(ctx._h, b.ptr, len(f), c.ptr, len(x) - 1, ctypes.byref(got)) == E_SPACE
    assert ctx.unpack_device(b, len(f), c, len(x)) == len(x) and c.download(len(x)).tobytes() == x


def test_host_forms(pkg, ctx):
    for x, w, block in ((f32_content(70001), 4, 0), (_u8(typed_input(5 * 4096 + 3, 4)), 8, 4096)):
        want = P.pack(x, w, block)
        f = ctx.pack(x, block, planes=w)
        assert f.tobytes() == want
        assert ctx.unpack(f).tobytes() == x.tobytes()
        assert pkg.unpack_size(f) == (x.size, f.size)
        with pytest.raises(pkg.BwtsError) as e:
            ctx.pack(x, block, out_cap=len(want) - 16, planes=w)
        assert e.value.code == E_SPACE
    # a failed unpack leaves out as it was
    x, f, cases = malformed_cases()
    for name, bad, code in cases:
        if name in ("two blocks swapped", "stream magic changed", "cut by 16", "width 4 rewritten to 2", "width word 3", "two entries with different widths"):
            out = np.full(len(x) + 16, 0x5A, dtype=np.uint8)
            with pytest.raises(pkg.BwtsError) as e:
                ctx.unpack(bad, out=out)
            assert e.value.code == code, name
            assert (out == 0x5A).all(), name
    out = np.full(len(x) - 1, 0x5A, dtype=np.uint8)
    with pytest.raises(pkg.BwtsError) as e:
        ctx.unpack(f, out=out)
    assert e.value.code == E_SPACE and (out == 0x5A).all()


def test_memory_kept(pkg):
    """device_bytes after a version-3 pack and after the unpack of its frame are version 2's: two n-byte blocks for a pack, one for
    an unpack, and no more.  (What the transform takes depends on the bytes it sees, so version 2 packs the split bytes here.)"""
    n = (1 << 20) + 1
    x = f32_content(n)
    kept = []
    for kw, data in (({"version": 2}, S.split(x, 4)), ({"planes": 4}, x)):
        with pkg.Context(0) as c:
            a, s, back = c.alloc(n), c.alloc(pkg.pack_bound(n, 0, **kw)), c.alloc(n)
            a.upload(data)
            size = c.pack_device(a, n, 0, s, s.nbytes, **kw)
            packed = c.timings().device_bytes
            c.release_memory()
            assert c.unpack_device(s, size, back, n) == n and np.array_equal(back.download(n), data)
            kept.append((packed, c.timings().device_bytes))
    assert kept[0] == kept[1], kept
    # ... and at most 2 n + 1 MiB more than the five single calls leave on a context of their own
    with pkg.Context(0) as c:
        a, b, s = c.alloc(n), c.alloc(n), c.alloc(pkg.pack_bound(n, 0, planes=4))
        a.upload(x)
        c.planes_split_device(a, n, 4, b)
        c.forward_device(b, n, a)
        c.mtf_forward_device(a, n, b)
        m = c.zrl_encode_device(b, n, a, n)
        c.ec_encode_device(a, m, s, s.nbytes)
        single = c.timings().device_bytes
    assert 2 * n <= kept[1][0] - single <= 2 * n + (1 << 20), (kept, single)


# -- the two CLIs, each run as a fresh child process ----------------------------------------------------------
@pytest.mark.parametrize("opts,w,block", [(["-p", "4", "-b", "64"], 4, 65536), (["-b", "4", "-p", "2"], 2, 4096)])
def test_cli_round_trip(tmp_path, opts, w, block):
    src = os.path.join(PKG_DIR, "testdata", "testjunk")
    data = open(src, "rb").read()
    packed, back = tmp_path / "junk.bwz", tmp_path / "junk.out"
    r = _run("bwts_pack", *opts, src, packed)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    frame = packed.read_bytes()
    assert frame == P.pack(data, w, block) and frame[4] == 3
    r = _run("bwts_unpack", packed, back)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert subprocess.run(["cmp", src, str(back)]).returncode == 0


def test_cli_usage():
    """(no device is opened: the options are judged first)"""
    for args in (["-p"], ["-p", "4"], ["-b", "4", "-p"]):
        r = _run("bwts_pack", *args)
        assert r.returncode == 1 and r.stderr.startswith(b"Usage: bwts_pack"), (args, r.stderr)
    for bad in ("3", "0", "16", "4x"):
        r = _run("bwts_pack", "-p", bad, os.path.join(PKG_DIR, "testdata", "testjunk"))
        assert r.returncode == 1 and b"width" in r.stderr, (bad, r.stderr)
