"""CPU model of version 3 of the member frame (include/bwts_members.h): a method per member beside its width and its filter.  The word at
entry offset 12 holds the width in bits 0-7, the filter in bits 8-15 and the method in bits 16-23 (0: the chain of versions 1 and 2;
1: the member's planes coded directly -- (delta,) split, coder).  A method-1 member is cut into coder segments by segments(): every
plane of a long member is a stream of its own, and the sizes of a member's several streams lie in the extension table behind the
entries, whose 8-byte words the header counts in the upper half of its count word.  The frame is canonical: a pack without a method
is the frame of pack_members_v2_model, byte for byte, and a version-3 frame in which no entry names a method is refused.  Every reader
takes all three versions here; a frame under the magic "BWTZ" goes where pack_members_model sends it."""
import bisect
import struct
import zlib

import delta_model as D
import ec_model as E
import pack_members_model as MM
import pack_members_v2_model as M2
import pack_range_model as R
import pack_v2_model as P2
import zrl_model as Z
from pack_model import E_ARG, E_CHECKSUM, E_FORMAT, E_RANGE, E_SPACE, MAX_N, PackError

VERSION_3 = 3
HEADER, ENTRY = MM.HEADER, MM.ENTRY
CHAIN, ORDER0 = 0, 1
METHODS = (CHAIN, ORDER0)
PLANE_MIN = 8192            # elements from which the planes of a direct member are coded apart


def word(w, f, m):
    return w | f << 8 | m << 16


def segments(ln, w):
    """The cut rule: the lengths of the coder segments of a method-1 member of ln bytes and width w."""
    q = ln // w
    if w > 1 and q >= PLANE_MIN:
        return [q] * (w - 1) + [q + (ln - q * w)]
    return [ln]


def table_words(ln, w, m):
    """The words a member has in the extension table: one per stream where it has several."""
    segs = segments(ln, w) if m == ORDER0 else [ln]
    return len(segs) if len(segs) > 1 else 0


def ext_words(lengths, widths, methods):
    """The 8-byte words of the extension table, the pad word that makes them even among them."""
    words = sum(table_words(ln, w, m) for ln, w, m in zip(lengths, widths, methods))
    return words + (words & 1)


def check_args(lengths, widths, filters, methods):
    """What a pack is asked for: widths (None: all 1), filters (None: none), methods (None: all 0) and n, or the refusal."""
    if lengths is None or len(lengths) == 0:
        raise PackError(E_ARG, "no members")
    if len(lengths) > MM.MAX_COUNT:
        raise PackError(E_RANGE, "more than 2^20 members")
    widths = [1] * len(lengths) if widths is None else list(widths)
    filters = [0] * len(lengths) if filters is None else list(filters)
    methods = [0] * len(lengths) if methods is None else list(methods)
    if (len(widths) != len(lengths) or len(filters) != len(lengths) or len(methods) != len(lengths) or any(ln == 0 for ln in lengths)
            or any(w not in MM.WIDTHS for w in widths) or any(f not in D.FILTERS for f in filters) or any(m not in METHODS for m in methods)):
        raise PackError(E_ARG, "a zero length, a bad width, a bad filter or a bad method")
    if sum(lengths) > MAX_N:
        raise PackError(E_RANGE, "more than 2^32 bytes")
    return widths, filters, methods, sum(lengths)


def bound(lengths, widths=None, methods=None):
    """bwts_pack_members_bound_m; 0 on bad arguments."""
    try:
        widths, _, methods, _ = check_args(lengths, widths, None, methods)
    except PackError:
        return 0
    total = HEADER + ENTRY * len(lengths) + 8 * ext_words(lengths, widths, methods)
    for ln, w, m in zip(lengths, widths, methods):
        total += sum(E.bound(s) for s in (segments(ln, w) if m == ORDER0 else [ln]))
    return total


def assemble(n, count, entries, table, streams, version=VERSION_3, ext=None):
    """A frame from (stream_bytes, crc, word, coded_bytes, len) entries, the table's words (the pad word among them) and the streams'
    bytes, with both header CRCs right.  ext: what the header says of the table, where that is not its length."""
    directory = b"".join(struct.pack("<QIIQQ", *e) for e in entries) + b"".join(struct.pack("<Q", t) for t in table)
    head = struct.pack("<IIQIII", MM.MAGIC, version, n, count, len(table) if ext is None else ext, zlib.crc32(directory))
    return head + struct.pack("<I", zlib.crc32(head)) + directory + b"".join(streams)


def direct_segments(m, w):
    """The coder segments of a method-1 member whose (filtered) bytes are m: its split bytes, cut by the rule."""
    y = MM.split(m, w).tobytes()
    out, at = [], 0
    for s in segments(len(m), w):
        out.append(y[at:at + s])
        at += s
    return out


def pack(members, widths=None, filters=None, methods=None):
    members = [bytes(m) for m in members]
    widths, filters, methods, n = check_args([len(m) for m in members], widths, filters, methods)
    if not any(methods):
        return M2.pack(members, widths, filters)
    front = [D.encode(m, w).tobytes() if f else m for m, w, f in zip(members, widths, filters)]
    # every direct segment is coded alone; the coder's segment form does that for all of them in one go (the bytes are E.encode's)
    segs = [direct_segments(fm, w) if md == ORDER0 else [] for fm, w, md in zip(front, widths, methods)]
    flat = [s for ss in segs for s in ss]
    coded_segs = iter(E.encode_segments(b"".join(flat), [len(s) for s in flat]))
    entries, table, streams = [], [], []
    for m, fm, w, f, md, sg in zip(members, front, widths, filters, methods, segs):
        if md == ORDER0:
            ss = [bytes(next(coded_segs)) for _ in sg]
            coded = len(m)
            if len(ss) > 1:
                table += [len(s) for s in ss]
        else:
            c = Z.encode(P2.ranks(MM.split(fm, w).tobytes()))
            ss, coded = [E.encode(c)], len(c)
        entries.append((sum(len(s) for s in ss), zlib.crc32(m), word(w, f, md), coded, len(m)))
        streams += ss
    if len(table) & 1:
        table.append(0)
    return assemble(n, len(members), entries, table, streams)


def version_of(buf):
    return M2.version_of(buf)


def _stream_ok(sb, ln):
    return sb % 16 == 0 and E.fixed_bytes(ln) + 256 * E.tiles(ln) <= sb <= E.bound(ln)


def check(buf, exact=True):
    """Header and directory of the member frame at the start of buf, any version: (n, entries, frame_bytes) with entries =
    [(stream_bytes, crc, w, coded_bytes, len, filter, method, segment stream sizes)].  The order is that of include/bwts_members.h,
    checks 1 to 11."""
    buf = bytes(buf)
    if version_of(buf) != VERSION_3 or not MM.is_members(buf):
        n, entries, total = M2.check(buf, exact)
        return n, [e + (CHAIN, [e[0]]) for e in entries], total
    if len(buf) < HEADER + ENTRY or len(buf) % 16:
        raise PackError(E_FORMAT, "length")
    magic, version, n, count, ext, dcrc, hcrc = struct.unpack("<IIQIIII", buf[:HEADER])
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
    fixed = HEADER + ENTRY * count + 8 * ext
    if fixed > len(buf):
        raise PackError(E_FORMAT, "directory longer than the frame")
    if dcrc != zlib.crc32(buf[HEADER:fixed]):
        raise PackError(E_FORMAT, "directory CRC")
    table = struct.unpack("<%dQ" % ext, buf[HEADER + ENTRY * count:fixed])
    entries, total, run, words = [], fixed, 0, 0
    for k in range(count):
        sb, crc, wfm, coded, ln = struct.unpack("<QIIQQ", buf[HEADER + ENTRY * k:HEADER + ENTRY * (k + 1)])
        w, f, m = wfm & 0xFF, (wfm >> 8) & 0xFF, (wfm >> 16) & 0xFF
        if w not in MM.WIDTHS or f not in D.FILTERS or m not in METHODS or wfm >> 24:
            raise PackError(E_FORMAT, "entry %d: width word" % k)
        if ln == 0 or ln > n - run:
            raise PackError(E_FORMAT, "entry %d: len" % k)
        run += ln
        if coded < 1 or coded > ln:
            raise PackError(E_FORMAT, "entry %d: coded_bytes" % k)
        if m == ORDER0 and coded != ln:
            raise PackError(E_FORMAT, "entry %d: a direct member's coded_bytes is its length" % k)
        tw = table_words(ln, w, m)
        if tw == 0:
            if not _stream_ok(sb, coded):
                raise PackError(E_FORMAT, "entry %d: no stream of that many coded bytes has that size" % k)
            sizes = [sb]
        else:
            if tw > ext - words:
                raise PackError(E_FORMAT, "entry %d: its table words reach beyond the table" % k)
            sizes = list(table[words:words + tw])
            if not all(_stream_ok(s, sl) for s, sl in zip(sizes, segments(ln, w))):
                raise PackError(E_FORMAT, "entry %d: no stream of a segment has that size" % k)
            if sum(sizes) != sb:
                raise PackError(E_FORMAT, "entry %d: the table words do not add up to stream_bytes" % k)
            words += tw
        entries.append((sb, crc, w, coded, ln, f, m, sizes))
        total += sb
    if not any(e[6] for e in entries):
        raise PackError(E_FORMAT, "version 3 and no entry names a method")
    if words + (words & 1) != ext:
        raise PackError(E_FORMAT, "ext is not what the entries demand")
    if words & 1 and table[words] != 0:
        raise PackError(E_FORMAT, "the pad word is not zero")
    if run != n:
        raise PackError(E_FORMAT, "the lengths do not add up to n")
    if total != len(buf) if exact else total > len(buf):
        raise PackError(E_FORMAT, "sizes do not add up to the frame")
    return n, entries, total


def fixed_of(buf):
    """Header, entries and extension table of a frame that passed check: where the streams begin."""
    buf = bytes(buf)
    if version_of(buf) != VERSION_3:
        return HEADER + ENTRY * struct.unpack("<Q", buf[16:24])[0]
    count, ext = struct.unpack("<II", buf[16:24])
    return HEADER + ENTRY * count + 8 * ext


def unpack_size(buf):
    if not MM.is_members(buf):
        return MM.unpack_size(buf)
    n, _, total = check(buf, exact=False)
    return n, total


def frame_members_m(buf):
    """bwts_frame_members_m: (lengths, widths, filters, methods); a "BWTZ" frame is refused."""
    _, entries, _ = check(buf, exact=True)
    return [e[4] for e in entries], [e[2] for e in entries], [e[5] for e in entries], [e[6] for e in entries]


def _direct_member(streams, sizes, w, ln):
    """A method-1 member's (filtered) bytes from its streams: every segment decoded against the length the cut gives it, then the join."""
    y, at = b"", 0
    for sb, sl in zip(sizes, segments(ln, w)):
        seg = E.decode(streams[at:at + sb], want_n=sl)
        if seg is None:
            raise PackError(E_FORMAT, "a segment's stream")
        y += bytes(seg)
        at += sb
    return MM.join(y, w).tobytes()


def _decode(frame, entries, which):
    """The members `which` (ascending), decoded whole, join and filter included, and held against their checksums, all of them before
    anything is made of one."""
    at = [fixed_of(frame)]
    for e in entries:
        at.append(at[-1] + e[0])
    out = []
    for k in which:
        sb, _, w, coded, ln, f, m, sizes = entries[k]
        if m == ORDER0:
            y = _direct_member(frame[at[k]:at[k] + sb], sizes, w, ln)
        else:
            y = MM._member(frame[at[k]:at[k] + sb], w, coded, ln)
        out.append(D.decode(y, w).tobytes() if f else bytes(y))
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


def covered(frame, ranges, out_cap=None):
    """The members a list of ranges touches, ascending, behind the frame's and the ranges' checks."""
    n, entries, _ = check(frame, exact=True)
    R.check_ranges(n, ranges, out_cap)
    off = [0]
    for e in entries:
        off.append(off[-1] + e[4])
    find = lambda at: bisect.bisect_right(off, at) - 1
    return sorted({b for o, nb in ranges for b in range(find(o), find(o + nb - 1) + 1)}), entries, off, find


def unpack_ranges(frame, ranges, out_cap=None):
    """The bytes of every range of the members' concatenation, a list in the order given; only covered members are decoded."""
    frame = bytes(frame)
    if not MM.is_members(frame):
        return MM.unpack_ranges(frame, ranges, out_cap)
    cov, entries, off, find = covered(frame, ranges, out_cap)
    got = dict(zip(cov, _decode(frame, entries, cov)))
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


def reseal(frame):
    """A version-3 frame with both header CRCs made right again for the count and ext its header names (as far as the frame holds the
    directory)."""
    frame = bytes(frame)
    count, ext = struct.unpack("<II", frame[16:24])
    fixed = min(HEADER + ENTRY * count + 8 * ext, len(frame))
    head = frame[:24] + struct.pack("<I", zlib.crc32(frame[HEADER:fixed]))
    return head + struct.pack("<I", zlib.crc32(head)) + frame[32:]
