"""CPU suite of the tensor-set layer and of the copy between scattered buffers (include/bwts_members.h, "Pointers"): tensor_frames on
hand-worked cuts, the tiling check of unpack_tensors on frames of tests/pack_members_v3_model.py (no device: the check comes before
any device call), and the edge arithmetic of scatter_pieces_kernel (csrc/pack_plan.h) under the sanitizers as a program of its own."""
import os
import shutil
import subprocess

import pytest

import members_v3_cases as C3
import pack_members_v3_model as M3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_FORMAT = -1, -8


def test_exact_fit_and_one_byte_over(pkg):
    tf = pkg.tensor_frames
    assert tf([40, 24], 64) == [[(0, 0, 40), (1, 0, 24)]]
    assert tf([40, 25], 64) == [[(0, 0, 40)], [(1, 0, 25)]]
    assert tf([64], 64) == [[(0, 0, 64)]]
    assert tf([64, 1], 64) == [[(0, 0, 64)], [(1, 0, 1)]]
    assert tf([30, 30, 4, 1, 63, 1], 64) == [[(0, 0, 30), (1, 0, 30), (2, 0, 4)], [(3, 0, 1), (4, 0, 63)], [(5, 0, 1)]]
    assert tf([], 64) == [] and tf([5]) == [[(0, 0, 5)]]
    assert tf([1 << 32, 1]) == [[(0, 0, 1 << 32)], [(1, 0, 1)]]


def test_a_tensor_of_three_frames_and_five_bytes(pkg):
    tf = pkg.tensor_frames
    n = 3 * 64 + 5
    whole = [[(1, 0, 64)], [(1, 64, 64)], [(1, 128, 64)]]
    # it closes the frame before it, and its last piece opens a frame that later tensors join
    assert tf([10, n, 50, 9, 1], 64) == [[(0, 0, 10)]] + whole + [[(1, 192, 5), (2, 0, 50), (3, 0, 9)], [(4, 0, 1)]]
    assert tf([n], 64) == [[(0, 0, 64)], [(0, 64, 64)], [(0, 128, 64)], [(0, 192, 5)]]
    # the pieces are frame_bytes rounded down to a multiple of 8
    assert tf([150], 63) == [[(0, 0, 56)], [(0, 56, 56)], [(0, 112, 38)]]
    assert tf([17], 8) == [[(0, 0, 8)], [(0, 8, 8)], [(0, 16, 1)]]
    assert tf([128], 64) == [[(0, 0, 64)], [(0, 64, 64)]]
    assert tf([(1 << 33) + 3]) == [[(0, 0, 1 << 32)], [(0, 1 << 32, 1 << 32)], [(0, 1 << 33, 3)]]


def test_zero_length_tensors_are_in_no_frame(pkg):
    tf = pkg.tensor_frames
    assert tf([0, 5, 0, 0, 7, 0], 64) == [[(1, 0, 5), (4, 0, 7)]]
    assert tf([0, 0], 64) == [] and tf([0, 64, 0, 1], 64) == [[(1, 0, 64)], [(3, 0, 1)]]


def test_the_member_cap(pkg):
    """2^20 one-byte tensors fill a frame whatever room frame_bytes leaves; the next one opens another."""
    cap = 1 << 20
    assert pkg.MAX_MEMBERS == cap
    for fb in (1 << 32, cap + 100):
        frames = pkg.tensor_frames([1] * (cap + 3), fb)
        assert [len(f) for f in frames] == [cap, 3]
        assert frames[0][0] == (0, 0, 1) and frames[0][-1] == (cap - 1, 0, 1) and frames[1] == [(cap, 0, 1), (cap + 1, 0, 1), (cap + 2, 0, 1)]
    # where frame_bytes binds first the count rule is not reached
    assert [len(f) for f in pkg.tensor_frames([1] * 100, 64)] == [64, 36]


def test_bad_frame_bytes(pkg):
    for fb in (0, 7, (1 << 32) + 1, -8):
        with pytest.raises(pkg.BwtsError) as e:
            pkg.tensor_frames([1, 2], fb)
        assert e.value.code == E_ARG
    assert pkg.tensor_frames([1, 2], 8) == [[(0, 0, 1), (1, 0, 2)]]
    assert pkg.tensor_frames([1, 2], 1 << 32) == [[(0, 0, 1), (1, 0, 2)]]


# -- the tiling check of unpack_tensors -----------------------------------------------------------------------------------
class HostTensor:
    """What unpack_tensors asks of a tensor, with no device behind it: any device call would fail on its address."""

    def __init__(self, nbytes, itemsize=1, contiguous=True):
        self.nbytes, self.itemsize, self.contiguous = nbytes, itemsize, contiguous

    def data_ptr(self):
        raise AssertionError("the tiling is judged before any device call")

    def element_size(self):
        return self.itemsize

    def numel(self):
        return self.nbytes // self.itemsize

    def is_contiguous(self):
        return self.contiguous


def model_frame(lengths):
    spec = [(ln, 1, 0, 1) for ln in lengths]
    return M3.pack(*C3.make_set(spec, 11))


def no_device_context(pkg):
    """A Context that was never given a device: every device call fails, the checks in front of them do not."""
    return pkg.Context.__new__(pkg.Context)


def test_members_must_tile_the_tensors(pkg):
    frames = [model_frame([100, 60]), model_frame([40, 7])]
    assert [pkg.frame_members(f)[0] for f in frames] == [[100, 60], [40, 7]]
    lens = [pkg.frame_members(f)[0] for f in frames]
    # two tensors cut as pack_tensors cuts them, zero-length tensors anywhere
    assert pkg.tensor_places(lens, [100, 100, 7]) == [[(0, 0, 100), (1, 0, 60)], [(1, 60, 40), (2, 0, 7)]]
    assert pkg.tensor_places(lens, [0, 100, 0, 100, 7, 0]) == [[(1, 0, 100), (3, 0, 60)], [(3, 60, 40), (4, 0, 7)]]
    assert pkg.tensor_places(lens, [207]) == [[(0, 0, 100), (0, 100, 60)], [(0, 160, 40), (0, 200, 7)]]
    ctx = no_device_context(pkg)
    bad = {"a member straddles two tensors": [99, 101, 7], "a member longer than its tensor": [100, 59, 48], "the tensors hold more": [100, 100, 8],
           "a tensor too many": [100, 100, 7, 1], "the tensors hold less": [100, 100], "no tensors": [], "the last member straddles": [100, 100, 6, 1]}
    for name, sizes in bad.items():
        with pytest.raises(pkg.BwtsError) as e:
            pkg.tensor_places(lens, sizes)
        assert e.value.code == E_ARG, name
        with pytest.raises(pkg.BwtsError) as e:
            ctx.unpack_tensors(frames, [HostTensor(b) for b in sizes])
        assert e.value.code == E_ARG, name
    # a tensor's bytes are its elements times their size: 13 elements of 8 bytes hold 104 bytes, four more than the members bring
    with pytest.raises(pkg.BwtsError) as e:
        ctx.unpack_tensors(frames, [HostTensor(100, 4), HostTensor(104, 8), HostTensor(7)])
    assert e.value.code == E_ARG
    with pytest.raises(pkg.BwtsError) as e:
        ctx.unpack_tensors(frames, [HostTensor(100), HostTensor(100, contiguous=False), HostTensor(7)])
    assert e.value.code == E_ARG
    with pytest.raises(pkg.BwtsError) as e:
        ctx.pack_tensors([HostTensor(100), HostTensor(100, contiguous=False)])
    assert e.value.code == E_ARG
    # a frame that is not a member frame is refused by its own check, before the tiling
    with pytest.raises(pkg.BwtsError) as e:
        ctx.unpack_tensors([frames[0][:-16]], [HostTensor(160)])
    assert e.value.code == E_FORMAT


def test_the_new_calls_are_declared_and_exported(pkg):
    new = {"bwts_gather_device", "bwts_scatter_device", "bwts_pack_members_p_device", "bwts_unpack_members_p_device"}
    assert new <= set(pkg.MEMBERS_EXPORTS) and not [s for s in new if not hasattr(pkg.lib(), s)]
    L = pkg.lib()
    assert L.bwts_gather_device(None, None, None, 1, None) == E_ARG and L.bwts_scatter_device(None, None, None, None, 1) == E_ARG
    assert L.bwts_pack_members_p_device(None, None, None, None, None, None, 1, None, 0, None, None, None) == E_ARG
    assert L.bwts_unpack_members_p_device(None, None, 64, None, 1, None, None) == E_ARG


# -- the kernel's edge arithmetic under the sanitizers, as a program of its own -----------------------------------------------
def test_scatter_edges_under_sanitizers(tmp_path):
    """tests/pieces_scatter_check.cc renders the accesses of scatter_pieces_kernel serially from pack_plan.h's arithmetic, over all
    16 x 16 misalignments and lengths 1 .. 49, T - 1, T, T + 1 and 2 T + 1: no access leaves its piece or is misaligned."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pieces_scatter_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "pieces_scatter_check.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, (r.stdout.decode(errors="replace")[-1000:], r.stderr.decode(errors="replace")[-2000:])
    assert r.stdout.decode().strip().endswith("checks ok")
