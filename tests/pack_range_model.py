"""CPU model of a range read of a packed frame (include/bwts_pack.h, "Ranges"): plan() says which blocks a list of (offset, bytes)
ranges covers and what is moved for them, unpack_ranges() decodes the covered blocks alone and cuts the ranges out.  Both judge the
frame with pack_v3_model.check (every version), then the ranges, and refuse with the library's codes in the library's order: the
executable form of the contract."""
import zlib

import numpy as np

import ec_model as E
import mtf_model as M
import oracle_lib as O
import pack_v3_model as P
import planes_model as S
import zrl_model as Z
from pack_model import E_ARG, E_CHECKSUM, E_FORMAT, E_RANGE, E_SPACE, HEADER, PackError, lengths

MAX_RANGES = 1 << 20
MAX_BYTES = 1 << 32
T = 16384               # the tile of copy_pieces_kernel (pack_plan.h: PIECES_T)


def check_ranges(n, ranges, out_cap=None):
    """The ranges of a call against a judged frame of n bytes: their sum, or the refusal."""
    if ranges is None or len(ranges) == 0:
        raise PackError(E_ARG, "no ranges")
    if len(ranges) > MAX_RANGES:
        raise PackError(E_RANGE, "more than 2^20 ranges")
    if any(b == 0 for _, b in ranges):
        raise PackError(E_ARG, "a range of no bytes")
    for off, b in ranges:
        if off + b >= 1 << 64 or off + b > n:
            raise PackError(E_RANGE, "range (%d, %d) leaves the input" % (off, b))
    total = sum(b for _, b in ranges)
    if total > MAX_BYTES:
        raise PackError(E_RANGE, "more than 2^32 bytes")
    if out_cap is not None and total > out_cap:
        raise PackError(E_SPACE, "sum > out_cap")
    return total


def plan(frame, ranges, out_cap=None):
    """What a range read decodes and moves, in the shape of the library's debug_unpack_ranges_plan (without T): the covered blocks as
    sorted maximal runs, the covered bytes, streams' bytes and coded bytes, one stream piece (offset in the frame, offset in the
    gathered streams, bytes) per run and one output piece (offset in the covered-block buffer, offset in the output, bytes) per range."""
    frame = bytes(frame)
    version, n, B, entries, _, width = P.check(frame, exact=True)
    total = check_ranges(n, ranges, out_cap)
    ls = lengths(n, B)
    covered = sorted({b for off, nb in ranges for b in range(off // B, (off + nb - 1) // B + 1)})
    runs = []
    for b in covered:
        if runs and runs[-1][0] + runs[-1][1] == b:
            runs[-1][1] += 1
        else:
            runs.append([b, 1])
    fixed = HEADER + (16 if version == 1 else 32) * len(ls)
    stream_at = [fixed]
    for sb, _, _ in entries:
        stream_at.append(stream_at[-1] + sb)
    at, c = {}, 0
    for b in covered:
        at[b] = c
        c += ls[b]
    streams, gathered = [], 0
    for first, blocks in runs:
        nbytes = stream_at[first + blocks] - stream_at[first]
        streams.append((stream_at[first], gathered, nbytes))
        gathered += nbytes
    out, dst = [], 0
    for off, nb in ranges:
        out.append((at[off // B] + off % B, dst, nb))
        dst += nb
    return {"blocks": len(covered), "runs": [tuple(r) for r in runs], "covered_bytes": c, "stream_bytes": gathered,
            "coded_bytes": sum(entries[b][2] for b in covered), "out_bytes": total, "streams": streams, "out": out,
            "covered": covered, "version": version, "width": width, "lengths": ls, "entries": entries, "stream_at": stream_at}


def decode_block(version, width, stream, coded, ln):
    """One block's bytes from its stream, through the stages of its version; the stages' refusals are E_FORMAT."""
    z = E.decode(stream, want_n=coded)
    if z is None:
        raise PackError(E_FORMAT, "stream")
    if version != 1:
        z = Z.decode(z, ln)
        if z is None:
            raise PackError(E_FORMAT, "zero-run input")
    x = O.inverse(np.frombuffer(M.inverse_fast(z), dtype=np.uint8))
    return (S.join(x, width) if version == 3 else x).tobytes()


def unpack_ranges(frame, ranges, out_cap=None):
    """The bytes of every range, a list in the order given.  Only covered blocks are decoded and only their checksums are held against
    the directory, all of them before anything is cut out."""
    frame = bytes(frame)
    p = plan(frame, ranges, out_cap)
    blocks = []
    for b in p["covered"]:
        sb, _, coded = p["entries"][b]
        blocks.append(decode_block(p["version"], p["width"], frame[p["stream_at"][b]:p["stream_at"][b] + sb], coded, p["lengths"][b]))
    for b, block in zip(p["covered"], blocks):
        if zlib.crc32(block) != p["entries"][b][1]:
            raise PackError(E_CHECKSUM, "block %d" % b)
    buf = b"".join(blocks)
    return [buf[src:src + nb] for src, _, nb in p["out"]]


# -- the range sets the suites share ------------------------------------------------------------------------------
def range_sets(n, B):
    """(name, ranges) for an input of n bytes in blocks of B: the named cases of the contract; those that need several blocks are left
    out where there is one."""
    nblk = -(-n // B)
    sets = [("first byte", [(0, 1)]), ("last byte", [(n - 1, 1)]), ("whole input", [(0, n)]), ("the same range twice", [(0, 1), (0, 1)])]
    if n > 2:
        sets += [("overlapping", [(0, n - 1), (1, n - 1)]), ("descending", [(n - 1, 1), (n // 2, 1), (0, 1)])]
    if nblk >= 6:
        last = (nblk - 1) * B
        sets += [
            ("ends at a seam", [(B - 10, 10)]),
            ("begins at a seam", [(2 * B, 10)]),
            ("straddles a seam by a byte each side", [(3 * B - 1, 2)]),
            ("the last block alone", [(last, n - last)]),
            ("an uncovered block between two ranges", [(5, 100), (2 * B + 7, 100)]),
            ("three runs", [(B // 2, 10), (2 * B + 1, 17), (last - 1, 2)]),
            ("overlapping across seams", [(B - 5, B + 10), (B + 100, 2 * B), (B - 5, 6)]),
            ("descending blocks", [(4 * B + 3, 50), (2 * B + 3, 50), (3, 50)]),
        ]
    return sets
