"""CPU model of the packed frame, version 2 (include/bwts_pack.h): version 1's model (tests/pack_model.py) with the zero-run stage
(tests/zrl_model.py) between the ranks and the coder and the directory entries of 32 bytes.  pack() writes a frame, check() judges
header and directory of either version in the order the header states, unpack() goes all the way back; each refuses with the code
the library returns."""
import struct
import zlib

import numpy as np

import ec_model as E
import mtf_model as M
import oracle_lib as O
import pack_model as P1
import zrl_model as Z
from pack_model import E_ARG, E_CHECKSUM, E_FORMAT, E_RANGE, E_SPACE, HEADER, MAGIC, MAX_N, MIN_BLOCK, PackError, block_len, lengths

VERSION = 2
ENTRY = 32


def bound(n, block_bytes=0, version=VERSION):
    if version == 1:
        return P1.bound(n, block_bytes)
    B = block_len(n, block_bytes)
    if B is None or version != VERSION:
        return 0
    return P1.bound(n, block_bytes) + (ENTRY - P1.ENTRY) * len(lengths(n, B))


def ranks(block):
    return np.frombuffer(M.forward_fast(O.forward(np.frombuffer(bytes(block), dtype=np.uint8)).tobytes()), dtype=np.uint8)


def assemble(n, B, entries, streams, version=VERSION):
    """A frame from (stream_bytes, crc, reserved, coded_bytes, reserved2) entries and the streams' bytes, with both header CRCs right."""
    d = b"".join(struct.pack("<QIIQQ", *e) for e in entries)
    h = struct.pack("<IIQQI", MAGIC, version, n, B, zlib.crc32(d))
    return h + struct.pack("<I", zlib.crc32(h)) + d + b"".join(streams)


def pack(data, block_bytes=0):
    data = bytes(data)
    B = block_len(len(data), block_bytes)
    if B is None:
        raise PackError(E_RANGE if len(data) > MAX_N else E_ARG, "bad arguments")
    blocks = [data[at:at + B] for at in range(0, len(data), B)]
    coded = [Z.encode(ranks(b)) for b in blocks]
    streams = [E.encode(c) for c in coded]
    return assemble(len(data), B, [(len(s), zlib.crc32(b), 0, len(c), 0) for s, b, c in zip(streams, blocks, coded)], streams)


def reseal(frame):
    """The frame with its two header CRCs recomputed over the header's n and B, with the entry size of the header's version (32 bytes
    unless it says 1), so that a change further in is reached by the checks behind the CRCs."""
    frame = bytes(frame)
    version, n, B = struct.unpack("<IQQ", frame[4:24])
    entry = P1.ENTRY if version == 1 else ENTRY
    nblk = -(-n // B) if B and 0 < n <= MAX_N else 0
    d = frame[HEADER:HEADER + entry * nblk]
    h = frame[:24] + struct.pack("<I", zlib.crc32(d))
    return h + struct.pack("<I", zlib.crc32(h)) + frame[HEADER:]


def check(buf, exact=True):
    """Header and directory of the frame at the start of buf, version 1 or 2, in the order of the header's list: (version, n, B,
    entries, frame_bytes) with entries = [(stream_bytes, crc, coded_bytes)] (version 1: coded_bytes is the block's length)."""
    buf = bytes(buf)
    if len(buf) < HEADER + P1.ENTRY or len(buf) % 16:
        raise PackError(E_FORMAT, "length")
    magic, version, n, B, dcrc, hcrc = struct.unpack("<IIQQII", buf[:HEADER])
    if magic != MAGIC or version not in (1, VERSION):
        raise PackError(E_FORMAT, "magic or version")
    if version == 1:
        n, B, entries, total = P1.check(buf, exact)
        return 1, n, B, [(sb, crc, ln) for (sb, crc), ln in zip(entries, lengths(n, B))], total
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
    entries, total = [], fixed
    for k, ln in enumerate(ls):
        sb, crc, rsv, coded, rsv2 = struct.unpack("<QIIQQ", buf[HEADER + ENTRY * k:HEADER + ENTRY * (k + 1)])
        if rsv != 0 or rsv2 != 0 or sb % 16:
            raise PackError(E_FORMAT, "entry %d" % k)
        if coded < 1 or coded > ln:
            raise PackError(E_FORMAT, "entry %d: coded_bytes" % k)
        if sb < E.fixed_bytes(coded) + 256 * E.tiles(coded) or sb > E.bound(coded):
            raise PackError(E_FORMAT, "entry %d: no stream of that many coded bytes has that size" % k)
        entries.append((sb, crc, coded))
        total += sb
    if total != len(buf) if exact else total > len(buf):
        raise PackError(E_FORMAT, "sizes do not add up to the frame")
    return version, n, B, entries, total


def unpack_size(buf):
    _, n, _, _, total = check(buf, exact=False)
    return n, total


def unpack(frame, out_cap=None):
    frame = bytes(frame)
    version, n, B, entries, _ = check(frame, exact=True)
    if version == 1:
        return P1.unpack(frame, out_cap)
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
        out.append(O.inverse(np.frombuffer(M.inverse_fast(r), dtype=np.uint8)).tobytes())
        at += sb
    for k, ((_, crc, _), block) in enumerate(zip(entries, out)):
        if zlib.crc32(block) != crc:
            raise PackError(E_CHECKSUM, "block %d" % k)
    return b"".join(out)
