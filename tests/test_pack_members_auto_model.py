"""CPU suite of the estimate and of the pack that chooses (include/bwts_members.h, "The estimate", "AUTO"): the models
(tests/estimate_model.py, tests/pack_members_auto_model.py) on the eleven inputs of DESIGN section 21 -- every row resolves to the
smallest cell of the section's table, the auto frame is the explicit frame of the resolved arrays, and the mixed frame beats each
uniform choice -- explicit values pass through, a tie goes to the chain, 255 stays refused by the version-3 model, the bound, the
library's host arithmetic, and the shared plan header under the sanitizers as a program of its own."""
import os
import re
import shutil
import struct
import subprocess

import pytest

import estimate_model as EST
import members_auto_cases as C
import pack_members_auto_model as A
import pack_members_model as MM
import pack_members_v3_model as M3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED_BYTES = 372512        # the model's frame of all eleven inputs, resolved per member


def code_of(fn, *args):
    try:
        fn(*args)
        return 0
    except MM.PackError as e:
        return e.code


def test_lg_and_costs():
    for k in range(32):
        assert EST.lg(1 << k) == k << 16
    assert EST.lg(3) == 103872 and EST.lg((1 << 32) - 1) == (32 << 16) - 1
    vals = [EST.lg(x) for x in range(1, 5000)]
    assert vals == sorted(vals)
    assert EST.hist_bytes([0] * 256) == 0 and EST.hist_bytes([7] + [0] * 255) == 0 and EST.hist_bytes([1024] * 256) == 1 << 18
    assert EST.hist_bytes([2048, 2048] + [0] * 254) == 512 and EST.hist_bytes([1, 1] + [0] * 254) == 1
    assert EST.units(0, 1) == 0 and EST.units(3, 4) == 0 and EST.units(4, 4) == 1 and EST.units(4 << 18, 4) == 1 and EST.units((4 << 18) + 4, 4) == 2
    assert EST.estimate(b"abc", 4) == (0, 0) and EST.estimate(bytes(4096), 2) == (0, 0)
    # a member's first element has 0 in front of it: the one difference that is not 0 costs each plane it touches two bytes
    assert EST.estimate(b"\x07\x07" * 4096, 2) == (0, 4) and EST.estimate(b"\x07\x00" * 4096, 2) == (0, 2)
    assert EST.choose_filter(65514, 65511) == 0 and EST.choose_filter(6400, 6299) == 1 and EST.choose_filter(6400, 6300) == 0 and EST.choose_filter(0, 0) == 0


def test_every_row_resolves_to_its_smallest_cell():
    for name, w, f, md, m in zip(C.NAMES, C.WIDTHS, C.FILTERS, C.ROWS, C.inputs()):
        fs, ms = A.resolve([m], [w])
        assert fs == [f], name
        # the filter is the one whose direct frame is smaller, in every row
        direct = [len(M3.pack([m], [w], [x], [1])) for x in (0, 1)]
        assert (direct[1] < direct[0]) == bool(f) or direct[0] == direct[1], name
        cells = {(x, y): len(M3.pack([m], [w], [x], [y])) for x in (0, 1) for y in (0, 1)}
        if md[3] is None:
            assert len(set(cells.values())) == 1 and ms == [0], name        # (all cells alike: the tie goes to the chain)
        else:
            assert ms == [md[3]] and cells[f, ms[0]] == min(cells.values()), (name, cells)
        # the auto frame is the model's explicit frame of the resolved arrays
        assert A.pack([m], [w]) == M3.pack([m], [w], fs, ms), name
    assert [C.FILTERS[i] for i in (1, 2, 6, 7)] == [0] * 4 and sum(C.FILTERS) == 7


def test_mixed_frame_beats_every_uniform_choice():
    members, widths = C.inputs(), C.WIDTHS
    fs, ms = A.resolve(members, widths)
    assert fs == C.FILTERS and ms == C.METHODS
    mixed = A.pack(members, widths)
    assert mixed == M3.pack(members, widths, fs, ms) and len(mixed) == MIXED_BYTES
    assert M3.unpack(mixed) == b"".join(members) and M3.frame_members_m(mixed) == ([C.BYTES] * 11, widths, fs, ms)
    for f in (0, 1):
        for md in (0, 1):
            assert len(mixed) < len(M3.pack(members, widths, [f] * 11, [md] * 11)), (f, md)
    assert len(mixed) <= A.bound([C.BYTES] * 11, widths)


def test_explicit_values_pass_through():
    members, widths = C.inputs()[:4], C.WIDTHS[:4]
    assert A.resolve(members, widths, [1, 0, 1, 0], [0, 0, 1, 1]) == ([1, 0, 1, 0], [0, 0, 1, 1])
    assert A.resolve(members, widths, 0, 1) == ([0] * 4, [1] * 4) and A.resolve(members, widths, None, None) == ([0] * 4, [0] * 4)
    # half the members explicit: the others as they resolve alone, and a method chosen at the filter that was named
    fs, ms = A.resolve(members, widths, [A.AUTO, 1, 0, A.AUTO], [1, A.AUTO, A.AUTO, 0])
    assert fs == [C.FILTERS[0], 1, 0, C.FILTERS[3]] and ms == [1, A.choose_method(*A.costs(members[1], 2, 1)), A.choose_method(*A.costs(members[2], 4, 0)), 0]
    assert A.pack(members, widths, [A.AUTO, 1, 0, A.AUTO], [1, A.AUTO, A.AUTO, 0]) == M3.pack(members, widths, fs, ms)
    assert A.pack(members, widths, 0, 0) == MM.pack(members, widths)


def test_a_tie_goes_to_the_chain():
    assert A.choose_method(1000, 1000) == 0 and A.choose_method(1000, 999) == 1 and A.choose_method(999, 1000) == 0
    # incompressible bytes: both encodings are the coder's bound, and a member of width 1 has no table words
    m = C.inputs()[7]
    chain, direct = A.costs(m, 1, 0)
    assert chain == direct and A.resolve([m], [1]) == ([0], [0])
    # the table's words count: a long member of width 4 pays 32 bytes for its four streams
    assert M3.table_words(C.BYTES, 4, 1) == 4
    m = C.inputs()[0]
    segs = M3.direct_segments(m, 4)
    assert A.costs(m, 4, 0)[1] == sum(len(s) for s in M3.E.encode_segments(b"".join(segs), [len(s) for s in segs])) + 32


def test_255_is_refused_where_it_always_was_and_the_bound():
    assert code_of(M3.check_args, [4], [4], [255], [0]) == MM.E_ARG and code_of(M3.check_args, [4], [4], [0], [255]) == MM.E_ARG
    assert code_of(A.check_args, [4], [4], [255], [255]) == 0 and code_of(A.check_args, [4], [4], [2], [0]) == MM.E_ARG
    assert code_of(A.check_args, [4], [4], [0], [254]) == MM.E_ARG and code_of(A.check_args, [4, 0], None, None, None) == MM.E_ARG
    assert code_of(A.check_args, [1 << 32, 1], None, [255, 255], None) == MM.E_RANGE
    ls, ws = [65536, 3, 32768, 32766, 800005], [4, 4, 2, 2, 8]
    for ms in ([255] * 5, [0, 255, 1, 255, 255], [255, 0, 0, 1, 1]):
        lo, hi = [0 if m == 255 else m for m in ms], [1 if m == 255 else m for m in ms]
        assert A.bound(ls, ws, ms) >= max(M3.bound(ls, ws, lo), M3.bound(ls, ws, hi))
    assert A.bound(ls, ws, [0, 1, 1, 0, 1]) == M3.bound(ls, ws, [0, 1, 1, 0, 1]) and A.bound(ls, ws, [0] * 5) == MM.bound(ls)
    assert A.bound(ls, ws, [0, 2, 0, 0, 0]) == 0 and A.bound([], None) == 0


# -- the library's host arithmetic and export list (no device) ----------------------------------------------------
def test_library_bound_and_exports(pkg):
    header = open(os.path.join(ROOT, "include", "bwts_members.h")).read()
    declared = set(re.findall(r"^(?:int|uint64_t) (bwts_[a-z0-9_]+)\(", header, flags=re.M))
    new = {"bwts_members_estimate_device", "bwts_members_estimate", "bwts_pack_members_bound_a", "bwts_pack_members_a_device", "bwts_pack_members_a"}
    assert new <= declared and declared == set(pkg.MEMBERS_EXPORTS)
    assert not [s for s in new if not hasattr(pkg.lib(), s)]
    assert re.search(r"#define BWTS_FILTER_AUTO 255u", header) and re.search(r"#define BWTS_METHOD_AUTO 255u", header)
    assert (pkg.FILTER_AUTO, pkg.METHOD_AUTO) == (A.AUTO, A.AUTO)
    ls, ws = [65536, 3, 32768, 32766, 800005], [4, 4, 2, 2, 8]
    for ms in ([255] * 5, [0, 255, 1, 255, 255], [0, 1, 1, 0, 1], [0] * 5):
        assert pkg.pack_members_bound_auto(ls, ws, ms) == A.bound(ls, ws, ms)
    assert pkg.pack_members_bound_auto(ls, ws) == A.bound(ls, ws) and pkg.pack_members_bound_auto(ls, None, 0) == MM.bound(ls)
    for bad, code in ((([5, 0], None, 255), -1), (([4], [3], 255), -1), (([4], [4], [7]), -1), (([1 << 32, 1], None, 255), -5)):
        with pytest.raises(pkg.BwtsError) as e:
            pkg.pack_members_bound_auto(*bad)
        assert e.value.code == code
    # the calls that take no AUTO refuse it as they always did
    with pytest.raises(pkg.BwtsError) as e:
        pkg.pack_members_bound(ls, ws, [255] * 5)
    assert e.value.code == -1


# -- the shared plan header and the AUTO predicates under the sanitizers, as a program of its own ---------------------
def test_plan_header_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    table = str(tmp_path / "lg.bin")
    with open(table, "wb") as f:
        f.write(struct.pack("<%dI" % (1 << 18), *[EST.lg(x) for x in range(1, (1 << 18) + 1)]))
    exe = str(tmp_path / "estimate_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "bijective-bwt_amd", "csrc"), os.path.join(ROOT, "tests", "estimate_plan_check.cc"), "-o", exe])
    r = subprocess.run([exe, table], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env={"PATH": os.environ.get("PATH", "")})
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert lines[-1].endswith("checks ok")
    # the members the program made, made again here, and the model against the serial statement's answers
    est = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("est ")]
    assert len(est) == 24
    x, mask = 0x2545F4914F6CDD1D, (1 << 64) - 1
    for w, ln, e0, e1 in est:
        m = bytearray(ln)
        for i in range(ln):
            x = (x * 6364136223846793005 + 1442695040888963407) & mask
            m[i] = (i // w + ((x >> 60) & 3)) & 255 if i % w == 0 else (x >> 56) & (0xFF if (i // w) % 3 == 0 else 0x03)
        assert EST.estimate(bytes(m), w) == (e0, e1), (w, ln)
