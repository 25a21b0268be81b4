"""CPU model of the member frame (include/bwts_members.h): members of any lengths, each split at a width of its own (1: not at all), in
one frame under the magic "BWTM".  The stages are those of the version-3 model (oracle, planes_model, mtf_model, zrl_model, ec_model,
zlib.crc32).  pack() writes a frame, check() judges header and directory in the order the header states, unpack() goes all the way
back, unpack_ranges() and unpack_members() decode the covered members alone, plan() says what such a read moves; each refuses with
the code the library returns.  A frame under the magic "BWTZ" goes to the models of its own (pack_v3_model, pack_range_model)."""
import bisect
import struct
import zlib

import numpy as np

import pack_range_model as R
import pack_v2_model as P2
import pack_v3_model as P3
import ec_model as E
import planes_model as S
import zrl_model as Z
from pack_model import E_ARG, E_CHECKSUM, E_FORMAT, E_RANGE, E_SPACE, MAX_N, PackError

MAGIC = 0x4D545742          # "BWTM"
VERSION = 1
HEADER = 32
ENTRY = 32
WIDTHS = (1, 2, 4, 8)
MAX_COUNT = 1 << 20
COPY_T = 32768              # the tile of a copied (width 1) segment of the mixed-width kernels (planes_plan.h: PLANES_COPY_T)


def split(x, w):
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    return x if w == 1 else S.split(x, w)


def join(y, w):
    y = np.frombuffer(bytes(y), dtype=np.uint8)
    return y if w == 1 else S.join(y, w)


def split_segments(x, lengths, widths, f=split):
    """Every segment of x split on its own at its own width; the outputs lie where the inputs lay."""
    x = bytes(x)
    assert sum(lengths) == len(x) and len(widths) == len(lengths)
    out, at = [], 0
    for ln, w in zip(lengths, widths):
        out.append(f(x[at:at + ln], w).tobytes())
        at += ln
    return b"".join(out)


def join_segments(y, lengths, widths):
    return split_segments(y, lengths, widths, join)


def tiles(ln, w):
    """The tiles the mixed-width kernels give a segment."""
    t = COPY_T if w == 1 else S.E * w
    return -(-ln // t)


def check_args(lengths, widths):
    """What a pack is asked for: the widths (None: all 1) and n, or the refusal."""
    if lengths is None or len(lengths) == 0:
        raise PackError(E_ARG, "no members")
    if len(lengths) > MAX_COUNT:
        raise PackError(E_RANGE, "more than 2^20 members")
    widths = [1] * len(lengths) if widths is None else list(widths)
    if len(widths) != len(lengths) or any(ln == 0 for ln in lengths) or any(w not in WIDTHS for w in widths):
        raise PackError(E_ARG, "a zero length or a bad width")
    if sum(lengths) > MAX_N:
        raise PackError(E_RANGE, "more than 2^32 bytes")
    return widths, sum(lengths)


def bound(lengths):
    """bwts_pack_members_bound; 0 on bad arguments."""
    try:
        check_args(lengths, None)
    except PackError:
        return 0
    return HEADER + ENTRY * len(lengths) + sum(E.bound(ln) for ln in lengths)


def assemble(n, count, entries, streams, magic=MAGIC, version=VERSION):
    """A frame from (stream_bytes, crc, width, coded_bytes, len) entries and the streams' bytes, with both header CRCs right."""
    directory = b"".join(struct.pack("<QIIQQ", *e) for e in entries)
    head = struct.pack("<IIQQI", magic, version, n, count, zlib.crc32(directory))
    return head + struct.pack("<I", zlib.crc32(head)) + directory + b"".join(streams)


def pack(members, widths=None):
    members = [bytes(m) for m in members]
    widths, n = check_args([len(m) for m in members], widths)
    coded = [Z.encode(P2.ranks(split(m, w).tobytes())) for m, w in zip(members, widths)]
    streams = [E.encode(c) for c in coded]
    entries = [(len(s), zlib.crc32(m), w, len(c), len(m)) for s, m, w, c in zip(streams, members, widths, coded)]
    return assemble(n, len(members), entries, streams)


def reseal(frame):
    """The frame with both header CRCs made right again for the count its header names (as far as the frame holds the directory)."""
    frame = bytes(frame)
    count = struct.unpack("<Q", frame[16:24])[0]
    fixed = min(HEADER + ENTRY * count, len(frame))
    head = frame[:24] + struct.pack("<I", zlib.crc32(frame[HEADER:fixed]))
    return head + struct.pack("<I", zlib.crc32(head)) + frame[32:]


def is_members(buf):
    return len(buf) >= 4 and struct.unpack("<I", bytes(buf[:4]))[0] == MAGIC


def check(buf, exact=True):
    """Header and directory of the member frame at the start of buf: (n, entries, frame_bytes) with entries = [(stream_bytes, crc, w,
    coded_bytes, len)].  The order is that of include/bwts_members.h, checks 1 to 10."""
    buf = bytes(buf)
    if len(buf) < HEADER + ENTRY or len(buf) % 16:
        raise PackError(E_FORMAT, "length")
    magic, version, n, count, dcrc, hcrc = struct.unpack("<IIQQII", buf[:HEADER])
    if magic != MAGIC or version != VERSION:
        raise PackError(E_FORMAT, "magic or version")
    if hcrc != zlib.crc32(buf[:28]):
        raise PackError(E_FORMAT, "header CRC")
    if n == 0:
        raise PackError(E_FORMAT, "n = 0")
    if n > MAX_N:
        raise PackError(E_RANGE, "n > 2^32")
    if count == 0 or count > n:
        raise PackError(E_FORMAT, "count")
    if count > MAX_COUNT:
        raise PackError(E_RANGE, "count > 2^20")
    fixed = HEADER + ENTRY * count
    if fixed > len(buf):
        raise PackError(E_FORMAT, "directory longer than the frame")
    if dcrc != zlib.crc32(buf[HEADER:fixed]):
        raise PackError(E_FORMAT, "directory CRC")
    entries, total, run = [], fixed, 0
    for k in range(count):
        sb, crc, w, coded, ln = struct.unpack("<QIIQQ", buf[HEADER + ENTRY * k:HEADER + ENTRY * (k + 1)])
        if w not in WIDTHS:
            raise PackError(E_FORMAT, "entry %d: width" % k)
        if ln == 0 or ln > n - run:
            raise PackError(E_FORMAT, "entry %d: len" % k)
        run += ln
        if coded < 1 or coded > ln:
            raise PackError(E_FORMAT, "entry %d: coded_bytes" % k)
        if sb % 16 or sb < E.fixed_bytes(coded) + 256 * E.tiles(coded) or sb > E.bound(coded):
            raise PackError(E_FORMAT, "entry %d: no stream of that many coded bytes has that size" % k)
        entries.append((sb, crc, w, coded, ln))
        total += sb
    if run != n:
        raise PackError(E_FORMAT, "the lengths do not add up to n")
    if total != len(buf) if exact else total > len(buf):
        raise PackError(E_FORMAT, "sizes do not add up to the frame")
    return n, entries, total


def unpack_size(buf):
    if not is_members(buf):
        return P3.unpack_size(buf)
    n, _, total = check(buf, exact=False)
    return n, total


def frame_members(buf):
    """bwts_frame_members: (lengths, widths); a "BWTZ" frame is refused."""
    _, entries, _ = check(buf, exact=True)
    return [e[4] for e in entries], [e[2] for e in entries]


def _stream_at(entries):
    at = [HEADER + ENTRY * len(entries)]
    for e in entries:
        at.append(at[-1] + e[0])
    return at


def _decode(frame, entries, which):
    """The members `which` (ascending), decoded and held against their checksums, all of them before anything is made of one."""
    at = _stream_at(entries)
    out = []
    for k in which:
        sb, _, w, coded, ln = entries[k]
        out.append(_member(frame[at[k]:at[k] + sb], w, coded, ln))
    for k, m in zip(which, out):
        if zlib.crc32(m) != entries[k][1]:
            raise PackError(E_CHECKSUM, "member %d" % k)
    return out


def _member(stream, w, coded, ln):
    """One member's bytes from its stream: version 3's stages (pack_range_model.decode_block) up to the join, which is at w or none."""
    if w == 1:
        return R.decode_block(2, 0, stream, coded, ln)
    return R.decode_block(3, w, stream, coded, ln)


def unpack(frame, out_cap=None):
    frame = bytes(frame)
    if not is_members(frame):
        return P3.unpack(frame, out_cap)
    n, entries, _ = check(frame, exact=True)
    if out_cap is not None and n > out_cap:
        raise PackError(E_SPACE, "n > out_cap")
    return b"".join(_decode(frame, entries, list(range(len(entries)))))


def plan(frame, ranges, out_cap=None):
    """pack_range_model.plan for a member frame: the covered members are found by bisecting the prefix sums of the lengths."""
    frame = bytes(frame)
    if not is_members(frame):
        return R.plan(frame, ranges, out_cap)
    n, entries, _ = check(frame, exact=True)
    total = R.check_ranges(n, ranges, out_cap)
    off = [0]
    for e in entries:
        off.append(off[-1] + e[4])
    find = lambda at: bisect.bisect_right(off, at) - 1
    covered = sorted({b for o, nb in ranges for b in range(find(o), find(o + nb - 1) + 1)})
    runs = []
    for b in covered:
        if runs and runs[-1][0] + runs[-1][1] == b:
            runs[-1][1] += 1
        else:
            runs.append([b, 1])
    stream_at = _stream_at(entries)
    at, c = {}, 0
    for b in covered:
        at[b] = c
        c += entries[b][4]
    streams, gathered = [], 0
    for first, blocks in runs:
        nbytes = stream_at[first + blocks] - stream_at[first]
        streams.append((stream_at[first], gathered, nbytes))
        gathered += nbytes
    out, dst = [], 0
    for o, nb in ranges:
        b = find(o)
        out.append((at[b] + o - off[b], dst, nb))
        dst += nb
    return {"blocks": len(covered), "runs": [tuple(r) for r in runs], "covered_bytes": c, "stream_bytes": gathered,
            "coded_bytes": sum(entries[b][3] for b in covered), "out_bytes": total, "streams": streams, "out": out,
            "covered": covered, "entries": entries, "stream_at": stream_at, "offsets": off}


def unpack_ranges(frame, ranges, out_cap=None):
    """The bytes of every range of the members' concatenation, a list in the order given; only covered members are decoded."""
    frame = bytes(frame)
    if not is_members(frame):
        return R.unpack_ranges(frame, ranges, out_cap)
    p = plan(frame, ranges, out_cap)
    buf = b"".join(_decode(frame, p["entries"], p["covered"]))
    return [buf[src:src + nb] for src, _, nb in p["out"]]


def index_ranges(frame, indices):
    """The ranges that whole members stand for, judged behind the frame: E_ARG for none, E_RANGE for too many or one out of range."""
    frame = bytes(frame)
    if not is_members(frame):
        P3.check(frame, exact=True)
        raise PackError(E_FORMAT, "not a member frame")
    _, entries, _ = check(frame, exact=True)
    if indices is None or len(indices) == 0:
        raise PackError(E_ARG, "no indices")
    if len(indices) > R.MAX_RANGES:
        raise PackError(E_RANGE, "more than 2^20 indices")
    off = [0]
    for e in entries:
        off.append(off[-1] + e[4])
    if any(i >= len(entries) for i in indices):
        raise PackError(E_RANGE, "no such member")
    return [(off[i], entries[i][4]) for i in indices]


def unpack_members(frame, indices, out_cap=None):
    """bwts_unpack_members: the members named, in the order asked; any order, repeats allowed, each decoded once."""
    return unpack_ranges(frame, index_ranges(frame, indices), out_cap)
