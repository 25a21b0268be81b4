"""GPU suite of pack / unpack with frames of version 2 (include/bwts_pack.h): every frame byte for byte against the CPU model
(tests/pack_v2_model.py), the device's frame and the model's frame unpacked on the device back to the input, the capacity contract,
frames of both versions through the same unpack, the malformed version-2 frames (each refused by the model with the same code
first), the host forms, the memory the calls keep, and the CLIs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pack_model as P1
import pack_v2_model as P
from test_pack_gpu import CONTENTS, ONE_BLOCK_N, PKG_DIR, _first_diff, _run, _u8, content
from test_pack_v2_model import FIXTURES, GOLDEN, malformed_cases

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
TOP = (1 << 20) + 5


@pytest.fixture(scope="module")
def bufs(pkg, ctx):
    """a: input; b: frame, as large as the bound of the largest input; c: output"""
    a, c = ctx.alloc(TOP + 64), ctx.alloc(TOP + 64)
    b = ctx.alloc(pkg.pack_bound(TOP, 4096, version=2) + 64)
    yield a, b, c
    for d in (a, b, c):
        d.free()


def _checked(pkg, ctx, bufs, x, block_bytes, capacity=True):
    """The checks of one input: device frame == model frame, device unpack of both == x, exact capacity, capacity - 16."""
    x = _u8(x)
    n = x.size
    a, b, c = bufs
    want = _u8(P.pack(x, block_bytes))
    a.upload(x)
    size = ctx.pack_device(a, n, block_bytes, b, pkg.pack_bound(n, block_bytes, version=2), version=2)
    assert size == want.size, (n, block_bytes, size, want.size)
    y = b.download(size)
    assert np.array_equal(y, want), "pack n=%d B=%d: %s" % (n, block_bytes, _first_diff(y, want))
    assert ctx.timings().n == n
    assert ctx.unpack_device(b, size, c, n) == n
    back = c.download(n)
    assert np.array_equal(back, x), "unpack n=%d B=%d: %s" % (n, block_bytes, _first_diff(back, x))
    b.upload(want)                                          # the model's frame, not the device's
    c.upload(np.zeros(n, dtype=np.uint8) if x.any() else np.ones(n, dtype=np.uint8))
    assert ctx.unpack_device(b, want.size, c, n + 5) == n
    assert np.array_equal(c.download(n), x)
    assert ctx.timings().n == n
    if capacity:
        mark = np.full(size + 64, 0xA5, dtype=np.uint8)
        b.upload(mark)
        assert ctx.pack_device(a, n, block_bytes, b, size, version=2) == size                     # exact capacity
        assert np.array_equal(b.download(size + 64), np.concatenate((want, mark[size:])))
        b.upload(mark)
        got = ctypes.c_uint64(0)
        rc = pkg.lib().bwts_pack_device_v(ctx._h, 2, a.ptr, n, block_bytes, b.ptr, size - 16, ctypes.byref(got))
        assert rc == E_SPACE, (n, rc)
        assert np.array_equal(b.download(size + 64), mark), "BWTS_E_SPACE, but something was written"      # the marks, everywhere
    return want


@pytest.mark.parametrize("name", CONTENTS)
def test_one_block(pkg, ctx, bufs, name):
    for n in ONE_BLOCK_N:
        f = _checked(pkg, ctx, bufs, content(name, n), 0, capacity=n <= 65537)
        assert f[4:8].view("<u4")[0] == 2 and f[16:24].view("<u8")[0] == n                  # B = n


@pytest.mark.parametrize("block,n", [(4096, 3 * 4096 + 1), (65536, (1 << 20) + 5), (4097, 40 * 4097 + 9)])
def test_blocks(pkg, ctx, bufs, block, n):
    x = content("text", n)
    f = _checked(pkg, ctx, bufs, x, block)
    assert f[8:24].view("<u8").tolist() == [n, block]
    if n < (1 << 20):
        _checked(pkg, ctx, bufs, content("zipf", n), block, capacity=False)
        # blocks that are stored beside blocks that are coded
        mixed = x.copy()
        mixed[block:2 * block] = content("uniform256", block)
        _checked(pkg, ctx, bufs, mixed, block, capacity=False)


def test_golden_fixtures_unpack_on_the_device(ctx, bufs):
    a, b, c = bufs
    for name, (x, _) in FIXTURES.items():
        f = _u8(open(os.path.join(GOLDEN, name), "rb").read())
        b.upload(f)
        assert ctx.unpack_device(b, f.size, c, len(x)) == len(x)
        assert c.download(len(x)).tobytes() == x, name


def test_both_versions_through_the_same_call(pkg, ctx, bufs):
    a, b, c = bufs
    for x, block in ((content("text", 70001), 0), (content("text", 5 * 4096 + 3), 4096)):
        n = x.size
        a.upload(x)
        frames = []
        for version in (1, 2):
            size = ctx.pack_device(a, n, block, b, pkg.pack_bound(n, block, version=version), version=version)
            frames.append(b.download(size))
            c.upload(np.zeros(n, dtype=np.uint8))
            assert ctx.unpack_device(b, size, c, n) == n and np.array_equal(c.download(n), x)
        assert frames[0].tobytes() == P1.pack(x, block) and frames[1].tobytes() == P.pack(x, block)
        assert block or frames[1].size < frames[0].size        # (one block of text: the zero-run stage pays; 4 KiB blocks are mostly coder overhead)
        size = ctx.pack_device(a, n, block, b, pkg.pack_bound(n, block))                    # no version: version 1, as before
        assert np.array_equal(b.download(size), frames[0])
    got = ctypes.c_uint64(0)
    for version in (0, 3):
        assert pkg.lib().bwts_pack_device_v(ctx._h, version, a.ptr, 5000, 0, b.ptr, 1 << 20, ctypes.byref(got)) == E_ARG
        host = np.zeros(64, dtype=np.uint8)
        assert pkg.lib().bwts_pack_v(ctx._h, version, host.ctypes.data, 16, 0, host.ctypes.data, 64, ctypes.byref(got)) == E_ARG


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
    for x, block in ((content("text", 70001), 0), (content("zipf", 5 * 4096 + 3), 4096)):
        want = P.pack(x, block)
        f = ctx.pack(x, block, version=2)
        assert f.tobytes() == want
        assert ctx.unpack(f).tobytes() == x.tobytes()
        assert pkg.unpack_size(f) == (x.size, f.size)
        with pytest.raises(pkg.BwtsError) as e:
            ctx.pack(x, block, out_cap=len(want) - 16, version=2)
        assert e.value.code == E_SPACE
    # a failed unpack leaves out as it was
    x, f, cases = malformed_cases()
    for name, bad, code in cases:
        if name in ("two blocks swapped", "stream magic changed", "cut by 16", "valid stream of an invalid zero-run input", "stream names coded_bytes + 1"):
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
    """device_bytes after a version-2 pack is at most 2 n + 1 MiB more than the four single calls leave on a context of their own."""
    n = (1 << 20) + 1
    x = content("zipf", n)
    with pkg.Context(0) as one, pkg.Context(0) as two:
        held = []
        for c in (one, two):
            a, b, s = c.alloc(n), c.alloc(n), c.alloc(pkg.pack_bound(n, 0, version=2))
            a.upload(x)
            held.append((a, b, s))
        a, b, s = held[0]
        one.pack_device(a, n, 0, s, s.nbytes, version=2)
        packed = one.timings().device_bytes
        a, b, s = held[1]
        two.forward_device(a, n, b)
        two.mtf_forward_device(b, n, a)
        m = two.zrl_encode_device(a, n, b, n)
        two.ec_encode_device(b, m, s, s.nbytes)
        single = two.timings().device_bytes
        assert 2 * n <= packed - single <= 2 * n + (1 << 20), (packed, single)


# -- the two CLIs, each run as a fresh child process ----------------------------------------------------------
def test_cli_round_trip(tmp_path):
    src = os.path.join(PKG_DIR, "testdata", "testjunk")
    data = open(src, "rb").read()
    for opts, block in ((["-z"], 0), (["-z", "-b", "4"], 4096), (["-b", "4", "-z"], 4096)):
        packed, back = tmp_path / "junk.bwz", tmp_path / "junk.out"
        r = _run("bwts_pack", *opts, src, packed)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        frame = packed.read_bytes()
        assert frame == P.pack(data, block) and len(frame) < len(data)
        r = _run("bwts_unpack", packed, back)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert subprocess.run(["cmp", src, str(back)]).returncode == 0


def test_cli_concatenated_frames_of_both_versions(tmp_path):
    one, two = b"first input, " * 700, bytes(range(256)) * 40
    (tmp_path / "one").write_bytes(one)
    (tmp_path / "two").write_bytes(two)
    for name, opts in (("one", []), ("two", ["-z", "-b", "4"])):
        assert _run("bwts_pack", *opts, tmp_path / name, tmp_path / (name + ".bwz")).returncode == 0
    v1, v2 = (tmp_path / "one.bwz").read_bytes(), (tmp_path / "two.bwz").read_bytes()
    assert v1[4] == 1 and v2[4] == 2
    (tmp_path / "both.bwz").write_bytes(v1 + v2 + v1)
    r = _run("bwts_unpack", tmp_path / "both.bwz", tmp_path / "both.out")
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert (tmp_path / "both.out").read_bytes() == one + two + one


def test_cli_usage():
    for args in (["-z"], ["-z", "-b"], ["-b", "4", "-z"], ["-z", "a", "b", "c"]):
        r = _run("bwts_pack", *args)
        assert r.returncode == 1 and r.stderr.startswith(b"Usage: bwts_pack"), (args, r.stderr)
    r = _run("bwts_pack", "-z", "-b", "3", os.path.join(PKG_DIR, "testdata", "testjunk"))
    assert r.returncode == 1 and b"block size" in r.stderr
