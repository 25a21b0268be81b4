"""CPU model of the packed frame (include/bwts_pack.h, version 1): the executable form of the format, built from the oracle (the
transform), mtf_model, ec_model and zlib.crc32.  pack() writes a frame, check() judges header and directory in the order the header
states, unpack() goes all the way back and compares every block's CRC; each refuses with the code the library returns."""
import struct
import zlib

import numpy as np

import ec_model as E
import mtf_model as M
import oracle_lib as O

MAGIC = 0x5A545742
VERSION = 1
HEADER = 32
ENTRY = 16
MIN_BLOCK = 4096
MAX_N = 1 << 32
E_ARG, E_RANGE, E_FORMAT, E_SPACE, E_CHECKSUM = -1, -5, -8, -9, -10
POLY = 0xEDB88320


class PackError(Exception):
    def __init__(self, code, why):
        super().__init__("%d: %s" % (code, why))
        self.code = code


# -- CRC-32 as polynomial arithmetic: a register's bit 31 is the coefficient of x^0 ------------------------------
def _times_x(a):
    return (a >> 1) ^ (POLY if a & 1 else 0)


def gf_mul(a, b):
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = _times_x(b)
    return p


def xpow8(nbytes):
    """x^(8 nbytes) mod P."""
    r, sq = 0x80000000, 0x00800000
    while nbytes:
        if nbytes & 1:
            r = gf_mul(r, sq)
        sq = gf_mul(sq, sq)
        nbytes >>= 1
    return r


def crc32_combine(crc_a, crc_b, len_b):
    """crc32(A + B) from crc32(A), crc32(B) and len(B): the initial and final terms of the two finished values cancel."""
    return gf_mul(crc_a, xpow8(len_b)) ^ crc_b


# -- the frame -------------------------------------------------------------------------------------------
def block_len(n, block_bytes):
    """The B a pack of n bytes stores for the caller's block_bytes; None: bad arguments."""
    if n < 1 or n > MAX_N:
        return None
    if block_bytes == 0 or block_bytes >= n:
        return n
    return None if block_bytes < MIN_BLOCK else block_bytes


def lengths(n, B):
    nblk = -(-n // B)
    return [B] * (nblk - 1) + [n - B * (nblk - 1)]


def bound(n, block_bytes=0):
    B = block_len(n, block_bytes)
    if B is None:
        return 0
    ls = lengths(n, B)
    return HEADER + ENTRY * len(ls) + (len(ls) - 1) * E.bound(B) + E.bound(ls[-1])


def _stream(block):
    return E.encode(M.forward_fast(O.forward(block).tobytes()))


def assemble(n, B, entries, streams):
    """A frame from (stream_bytes, crc, reserved) entries and the streams' bytes, with both header CRCs right."""
    d = b"".join(struct.pack("<QII", sb, crc, rsv) for sb, crc, rsv in entries)
    h = struct.pack("<IIQQI", MAGIC, VERSION, n, B, zlib.crc32(d))
    return h + struct.pack("<I", zlib.crc32(h)) + d + b"".join(streams)


def pack(data, block_bytes=0):
    data = bytes(data)
    B = block_len(len(data), block_bytes)
    if B is None:
        raise PackError(E_RANGE if len(data) > MAX_N else E_ARG, "bad arguments")
    blocks = [data[at:at + B] for at in range(0, len(data), B)]
    streams = [_stream(np.frombuffer(b, dtype=np.uint8)) for b in blocks]
    return assemble(len(data), B, [(len(s), zlib.crc32(b), 0) for s, b in zip(streams, blocks)], streams)


def reseal(frame):
    """The frame with its two header CRCs recomputed over the header's n and B (as many directory bytes as they name, or as there
    are), so that a change further in is reached by the checks behind the CRCs."""
    frame = bytes(frame)
    n, B = struct.unpack("<QQ", frame[8:24])
    nblk = -(-n // B) if B and 0 < n <= MAX_N else 0
    d = frame[HEADER:HEADER + ENTRY * nblk]
    h = frame[:24] + struct.pack("<I", zlib.crc32(d))
    return h + struct.pack("<I", zlib.crc32(h)) + frame[HEADER:]


def check(buf, exact=True):
    """Header and directory of the frame at the start of buf, in the order of the header's list: (n, B, entries, frame_bytes) with
    entries = [(stream_bytes, crc)].  exact: the frame must be all of buf."""
    buf = bytes(buf)
    if len(buf) < HEADER + ENTRY or len(buf) % 16:
        raise PackError(E_FORMAT, "length")
    magic, version, n, B, dcrc, hcrc = struct.unpack("<IIQQII", buf[:HEADER])
    if magic != MAGIC or version != VERSION:
        raise PackError(E_FORMAT, "magic or version")
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
        sb, crc, rsv = struct.unpack("<QII", buf[HEADER + ENTRY * k:HEADER + ENTRY * (k + 1)])
        if rsv != 0 or sb % 16:
            raise PackError(E_FORMAT, "entry %d" % k)
        if sb < E.fixed_bytes(ln) + 256 * E.tiles(ln) or sb > E.bound(ln):
            raise PackError(E_FORMAT, "entry %d: no stream of this block has that size" % k)
        entries.append((sb, crc))
        total += sb
    if total != len(buf) if exact else total > len(buf):
        raise PackError(E_FORMAT, "sizes do not add up to the frame")
    return n, B, entries, total


def unpack_size(buf):
    n, _, _, total = check(buf, exact=False)
    return n, total


def unpack(frame, out_cap=None):
    frame = bytes(frame)
    n, B, entries, _ = check(frame, exact=True)
    if out_cap is not None and n > out_cap:
        raise PackError(E_SPACE, "n > out_cap")
    out, at = [], HEADER + ENTRY * len(entries)
    for (sb, _), ln in zip(entries, lengths(n, B)):
        ranks = E.decode(frame[at:at + sb], want_n=ln)
        if ranks is None:
            raise PackError(E_FORMAT, "stream")
        out.append(O.inverse(np.frombuffer(M.inverse_fast(ranks), dtype=np.uint8)).tobytes())
        at += sb
    for k, ((_, crc), block) in enumerate(zip(entries, out)):
        if zlib.crc32(block) != crc:
            raise PackError(E_CHECKSUM, "block %d" % k)
    return b"".join(out)
