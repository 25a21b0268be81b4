"""CPU model of version 2 of the member frame (include/bwts_members.h): a filter per member beside its width.  The word at entry offset
12 holds the width in bits 0-7 and the filter (delta_model: 0 none, 1 delta) in bits 8-15; a filtered member goes through
delta_model.encode at its width in front of the split, and its CRC-32 stays that of the original bytes.  The frame is canonical: a
pack without a filter is the version-1 frame of pack_members_model, byte for byte, and a version-2 frame in which no entry names a
filter is refused.  Every reader takes both versions here; a frame under the magic "BWTZ" goes where pack_members_model sends it."""
import bisect
import struct
import zlib

import delta_model as D
import ec_model as E
import pack_members_model as MM
import pack_range_model as R
import pack_v2_model as P2
import zrl_model as Z
from pack_model import E_ARG, E_CHECKSUM, E_FORMAT, E_RANGE, E_SPACE, MAX_N, PackError

VERSION_2 = 2
HEADER, ENTRY = MM.HEADER, MM.ENTRY
WALK_N = 1 << 18            # the size pin: 256 KiB


def walk_i32(n=WALK_N, seed=5):
    """The int32 random walk of the size table: steps uniform in [-50, 50], n bytes, numpy default_rng(seed)."""
    import numpy as np
    steps = np.random.default_rng(seed).integers(-50, 51, n // 4)
    return np.cumsum(steps).astype("<i4").tobytes()


def bf16_gaussian(n=WALK_N, seed=5):
    """Gaussian weights (sigma 0.02) as bfloat16, the upper halves of their float32: n bytes."""
    import numpy as np
    x = (np.random.default_rng(seed).standard_normal(n // 2) * 0.02).astype("<f4")
    return (x.view("<u4") >> 16).astype("<u2").tobytes()


def word(w, f):
    return w | (f << 8)


def check_args(lengths, widths, filters):
    """What a pack is asked for: widths (None: all 1), filters (None: none) and n, or the refusal."""
    if lengths is None or len(lengths) == 0:
        raise PackError(E_ARG, "no members")
    if len(lengths) > MM.MAX_COUNT:
        raise PackError(E_RANGE, "more than 2^20 members")
    widths = [1] * len(lengths) if widths is None else list(widths)
    filters = [0] * len(lengths) if filters is None else list(filters)
    if (len(widths) != len(lengths) or len(filters) != len(lengths) or any(ln == 0 for ln in lengths) or any(w not in MM.WIDTHS for w in widths)
            or any(f not in D.FILTERS for f in filters)):
        raise PackError(E_ARG, "a zero length, a bad width or a bad filter")
    if sum(lengths) > MAX_N:
        raise PackError(E_RANGE, "more than 2^32 bytes")
    return widths, filters, sum(lengths)


def assemble(n, count, entries, streams, version=VERSION_2):
    """A frame from (stream_bytes, crc, width word, coded_bytes, len) entries and the streams' bytes, with both header CRCs right."""
    return MM.assemble(n, count, entries, streams, version=version)


def pack(members, widths=None, filters=None):
    members = [bytes(m) for m in members]
    widths, filters, n = check_args([len(m) for m in members], widths, filters)
    if not any(filters):
        return MM.pack(members, widths)
    front = [D.encode(m, w).tobytes() if f else m for m, w, f in zip(members, widths, filters)]
    coded = [Z.encode(P2.ranks(MM.split(m, w).tobytes())) for m, w in zip(front, widths)]
    streams = [E.encode(c) for c in coded]
    entries = [(len(s), zlib.crc32(m), word(w, f), len(c), len(m)) for s, m, w, f, c in zip(streams, members, widths, filters, coded)]
    return assemble(n, len(members), entries, streams)


def version_of(buf):
    return struct.unpack("<I", bytes(buf[4:8]))[0] if len(buf) >= 8 else 0


def check(buf, exact=True):
    """Header and directory of the member frame at the start of buf, either version: (n, entries, frame_bytes) with entries =
    [(stream_bytes, crc, w, coded_bytes, len, filter)].  The order is that of include/bwts_members.h, checks 1 to 11."""
    buf = bytes(buf)
    if len(buf) < HEADER + ENTRY or len(buf) % 16:
        raise PackError(E_FORMAT, "length")
    magic, version, n, count, dcrc, hcrc = struct.unpack("<IIQQII", buf[:HEADER])
    if magic != MM.MAGIC or version not in (MM.VERSION, VERSION_2):
        raise PackError(E_FORMAT, "magic or version")
    if hcrc != zlib.crc32(buf[:28]):
        raise PackError(E_FORMAT, "header CRC")
    if n == 0:
        raise PackError(E_FORMAT, "n = 0")
    if n > MAX_N:
        raise PackError(E_RANGE, "n > 2^32")
    if count == 0 or count > n:
        raise PackError(E_FORMAT, "count")
    if count > MM.MAX_COUNT:
        raise PackError(E_RANGE, "count > 2^20")
    fixed = HEADER + ENTRY * count
    if fixed > len(buf):
        raise PackError(E_FORMAT, "directory longer than the frame")
    if dcrc != zlib.crc32(buf[HEADER:fixed]):
        raise PackError(E_FORMAT, "directory CRC")
    entries, total, run = [], fixed, 0
    for k in range(count):
        sb, crc, wf, coded, ln = struct.unpack("<QIIQQ", buf[HEADER + ENTRY * k:HEADER + ENTRY * (k + 1)])
        w, f = (wf, 0) if version == MM.VERSION else (wf & 0xFF, (wf >> 8) & 0xFF)
        if w not in MM.WIDTHS or f not in D.FILTERS or (version == VERSION_2 and wf >> 16):
            raise PackError(E_FORMAT, "entry %d: width word" % k)
        if ln == 0 or ln > n - run:
            raise PackError(E_FORMAT, "entry %d: len" % k)
        run += ln
        if coded < 1 or coded > ln:
            raise PackError(E_FORMAT, "entry %d: coded_bytes" % k)
        if sb % 16 or sb < E.fixed_bytes(coded) + 256 * E.tiles(coded) or sb > E.bound(coded):
            raise PackError(E_FORMAT, "entry %d: no stream of that many coded bytes has that size" % k)
        entries.append((sb, crc, w, coded, ln, f))
        total += sb
    if version == VERSION_2 and not any(e[5] for e in entries):
        raise PackError(E_FORMAT, "version 2 and no entry names a filter")
    if run != n:
        raise PackError(E_FORMAT, "the lengths do not add up to n")
    if total != len(buf) if exact else total > len(buf):
        raise PackError(E_FORMAT, "sizes do not add up to the frame")
    return n, entries, total


def unpack_size(buf):
    if not MM.is_members(buf):
        return MM.unpack_size(buf)
    n, _, total = check(buf, exact=False)
    return n, total


def frame_members_f(buf):
    """bwts_frame_members_f: (lengths, widths, filters); a "BWTZ" frame is refused."""
    _, entries, _ = check(buf, exact=True)
    return [e[4] for e in entries], [e[2] for e in entries], [e[5] for e in entries]


def _decode(frame, entries, which):
    """The members `which` (ascending), decoded whole, filter included, and held against their checksums, all of them before anything
    is made of one."""
    at = MM._stream_at(entries)
    out = []
    for k in which:
        sb, _, w, coded, ln, f = entries[k]
        m = MM._member(frame[at[k]:at[k] + sb], w, coded, ln)
        out.append(D.decode(m, w).tobytes() if f else bytes(m))
    for k, m in zip(which, out):
        if zlib.crc32(m) != entries[k][1]:
            raise PackError(E_CHECKSUM, "member %d" % k)
    return out


def unpack(frame, out_cap=None):
    frame = bytes(frame)
    if not MM.is_members(frame):
        return MM.unpack(frame, out_cap)
    n, entries, _ = check(frame, exact=True)
    if out_cap is not None and n > out_cap:
        raise PackError(E_SPACE, "n > out_cap")
    return b"".join(_decode(frame, entries, list(range(len(entries)))))


def unpack_ranges(frame, ranges, out_cap=None):
    """The bytes of every range of the members' concatenation, a list in the order given; only covered members are decoded."""
    frame = bytes(frame)
    if not MM.is_members(frame):
        return MM.unpack_ranges(frame, ranges, out_cap)
    n, entries, _ = check(frame, exact=True)
    R.check_ranges(n, ranges, out_cap)
    off = [0]
    for e in entries:
        off.append(off[-1] + e[4])
    find = lambda at: bisect.bisect_right(off, at) - 1
    covered = sorted({b for o, nb in ranges for b in range(find(o), find(o + nb - 1) + 1)})
    got = dict(zip(covered, _decode(frame, entries, covered)))
    out = []
    for o, nb in ranges:
        b, piece = find(o), b""
        while len(piece) < nb:
            piece += got[b][o + len(piece) - off[b]:][:nb - len(piece)]
            b += 1
        out.append(piece)
    return out


def unpack_members(frame, indices, out_cap=None):
    """bwts_unpack_members: the members named, in the order asked; any order, repeats allowed, each decoded once."""
    frame = bytes(frame)
    if not MM.is_members(frame):
        return MM.unpack_members(frame, indices, out_cap)
    _, entries, _ = check(frame, exact=True)
    if indices is None or len(indices) == 0:
        raise PackError(E_ARG, "no indices")
    if len(indices) > R.MAX_RANGES:
        raise PackError(E_RANGE, "more than 2^20 indices")
    if any(i >= len(entries) for i in indices):
        raise PackError(E_RANGE, "no such member")
    off = [0]
    for e in entries:
        off.append(off[-1] + e[4])
    return unpack_ranges(frame, [(off[i], entries[i][4]) for i in indices], out_cap)
