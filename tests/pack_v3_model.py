"""CPU model of the packed frame, version 3 (include/bwts_pack.h): version 2's model (tests/pack_v2_model.py) with the byte-plane split
(tests/planes_model.py) in front of the transform and the split's width in the word at entry offset 12, the reserved word of versions
1 and 2.  pack() writes a frame, check() judges header and directory of any version in the order the header states, unpack() goes
all the way back; each refuses with the code the library returns."""
import struct
import zlib

import numpy as np

import ec_model as E
import mtf_model as M
import oracle_lib as O
import pack_model as P1
import pack_v2_model as P2
import planes_model as S
import zrl_model as Z
from pack_model import E_ARG, E_CHECKSUM, E_FORMAT, E_RANGE, E_SPACE, HEADER, MAGIC, MAX_N, MIN_BLOCK, PackError, block_len, lengths

VERSION = 3
ENTRY = 32
WIDTHS = S.WIDTHS


def bound(width, n, block_bytes=0):
    """bwts_pack_planes_bound: version 2's bound; 0 for a bad width or bad block arguments."""
    return P2.bound(n, block_bytes) if width in WIDTHS else 0


def assemble(n, B, entries, streams, version=VERSION):
    """A frame from (stream_bytes, crc, width, coded_bytes, reserved2) entries and the streams' bytes, with both header CRCs right."""
    return P2.assemble(n, B, entries, streams, version)


def pack(data, width, block_bytes=0):
    data = bytes(data)
    B = block_len(len(data), block_bytes)
    if B is None or width not in WIDTHS:
        raise PackError(E_RANGE if len(data) > MAX_N else E_ARG, "bad arguments")
    blocks = [data[at:at + B] for at in range(0, len(data), B)]
    coded = [Z.encode(P2.ranks(S.split(b, width).tobytes())) for b in blocks]
    streams = [E.encode(c) for c in coded]
    return assemble(len(data), B, [(len(s), zlib.crc32(b), width, len(c), 0) for s, b, c in zip(streams, blocks, coded)], streams)


reseal = P2.reseal          # (32-byte entries for every version but 1)


def check(buf, exact=True):
    """Header and directory of the frame at the start of buf, version 1, 2 or 3: (version, n, B, entries, frame_bytes, width) with
    entries = [(stream_bytes, crc, coded_bytes)]; width is 0 for versions 1 and 2."""
    buf = bytes(buf)
    if len(buf) < HEADER + P1.ENTRY or len(buf) % 16:
        raise PackError(E_FORMAT, "length")
    magic, version, n, B, dcrc, hcrc = struct.unpack("<IIQQII", buf[:HEADER])
    if magic != MAGIC or version not in (1, 2, VERSION):
        raise PackError(E_FORMAT, "magic or version")
    if version != VERSION:
        return P2.check(buf, exact) + (0,)
    if hcrc != zlib.crc32(buf[:28]):
        raise PackError(E_FORMAT, "header CRC")
    if n == 0:
        raise PackError(E_FORMAT, "n = 0")
    if n > MAX_N:
        raise PackError(E_RANGE, "n > 2^32")
    if B == 0 or B > n or (B < MIN_BLOCK and B != n):
        raise PackError(E_FORMAT, "B")
    ls = lengths(n, B)
    fixed = HEADER + ENTRY * len(ls)
    if fixed > len(buf):
        raise PackError(E_FORMAT, "directory longer than the frame")
    if dcrc != zlib.crc32(buf[HEADER:fixed]):
        raise PackError(E_FORMAT, "directory CRC")
    width = struct.unpack("<I", buf[HEADER + 12:HEADER + 16])[0]
    entries, total = [], fixed
    for k, ln in enumerate(ls):
        sb, crc, w, coded, rsv2 = struct.unpack("<QIIQQ", buf[HEADER + ENTRY * k:HEADER + ENTRY * (k + 1)])
        if w != width or w not in WIDTHS or rsv2 != 0 or sb % 16:
            raise PackError(E_FORMAT, "entry %d" % k)
        if coded < 1 or coded > ln:
            raise PackError(E_FORMAT, "entry %d: coded_bytes" % k)
        if sb < E.fixed_bytes(coded) + 256 * E.tiles(coded) or sb > E.bound(coded):
            raise PackError(E_FORMAT, "entry %d: no stream of that many coded bytes has that size" % k)
        entries.append((sb, crc, coded))
        total += sb
    if total != len(buf) if exact else total > len(buf):
        raise PackError(E_FORMAT, "sizes do not add up to the frame")
    return version, n, B, entries, total, width


def unpack_size(buf):
    _, n, _, _, total, _ = check(buf, exact=False)
    return n, total


def unpack(frame, out_cap=None):
    frame = bytes(frame)
    version, n, B, entries, _, width = check(frame, exact=True)
    if version != VERSION:
        return P2.unpack(frame, out_cap)
    if out_cap is not None and n > out_cap:
        raise PackError(E_SPACE, "n > out_cap")
    out, at = [], HEADER + ENTRY * len(entries)
    for (sb, _, coded), ln in zip(entries, lengths(n, B)):
        z = E.decode(frame[at:at + sb], want_n=coded)
        if z is None:
            raise PackError(E_FORMAT, "stream")
        r = Z.decode(z, ln)
        if r is None:
            raise PackError(E_FORMAT, "zero-run input: %s" % Z.why())
        out.append(S.join(O.inverse(np.frombuffer(M.inverse_fast(r), dtype=np.uint8)), width).tobytes())
        at += sb
    for k, ((_, crc, _), block) in enumerate(zip(entries, out)):
        if zlib.crc32(block) != crc:
            raise PackError(E_CHECKSUM, "block %d" % k)
    return b"".join(out)


def f32_field(values, seed=1):
    """The smooth field of the size tables: sin(x) + 0.3 sin(7.1 x) + 1e-3 noise over `values` float32 numbers, as bytes."""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 20.0, values)
    return (np.sin(x) + 0.3 * np.sin(7.1 * x) + 1e-3 * rng.standard_normal(values)).astype("<f4").tobytes()


def bf16_gaussian(values, seed=2):
    """Gaussian weights rounded to bf16 (the upper halves of their float32 form), as bytes."""
    rng = np.random.default_rng(seed)
    w = (0.02 * rng.standard_normal(values)).astype("<f4").view("<u4")
    return ((w + 0x8000) >> 16).astype("<u2").tobytes()
