"""The host layer's plain C++ under the sanitizers, as a program of its own (no GPU, nothing loaded into Python): the copy workers
of csrc/copy_pool.h and the segment table's region arithmetic of csrc/seg_layout.h, driven by tests/host_layer_check.cc."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bijective-bwt_amd", "csrc")


@pytest.mark.parametrize("name,flags", [("thread", ["-fsanitize=thread"]),
                                        ("address", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_copy_pool_and_segment_layout_under_sanitizers(tmp_path, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / ("host_layer_check_" + name))
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-pthread"] + flags +
                          ["-I", CSRC, os.path.join(ROOT, "tests", "host_layer_check.cc"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, (r.stdout.decode(errors="replace")[-1000:], r.stderr.decode(errors="replace")[-3000:])
    assert r.stdout.decode().strip().endswith("checks ok")


def test_headers_are_plain_cxx():
    """Neither header may pull in the device runtime: the program above has to build with a host compiler alone."""
    for h in ("copy_pool.h", "seg_layout.h"):
        includes = [line for line in open(os.path.join(CSRC, h)).read().splitlines() if line.startswith("#include")]
        assert includes and not [line for line in includes if "hip" in line or "internal.h" in line], h
