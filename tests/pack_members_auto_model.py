"""CPU model of the pack that chooses (include/bwts_members.h, "AUTO"): a filter or a method of 255 is left to the writer, which resolves
it by two rules and then writes the frame that pack_members_v3_model.pack writes for the resolved arrays -- no version of its own, no
field of its own, and every reader as it was.
  A filter AUTO becomes delta iff est_delta + (est_none >> 6) < est_none (estimate_model), else none, whatever the member's method.
  A method AUTO: the member is encoded both ways at its resolved filter; a way costs its stream bytes and 8 bytes per word it has in
  the extension table; the smaller cost wins, and a tie goes to the chain."""
import functools

import delta_model as D
import ec_model as E
import estimate_model as EST
import pack_members_model as MM
import pack_members_v3_model as M3
import pack_v2_model as P2
import zrl_model as Z
from pack_model import E_ARG, E_RANGE, MAX_N, PackError

AUTO = 255
CHAIN, ORDER0 = M3.CHAIN, M3.ORDER0


def check_args(lengths, widths, filters, methods):
    """pack_members_v3_model.check_args with AUTO among the filters and the methods."""
    if lengths is None or len(lengths) == 0:
        raise PackError(E_ARG, "no members")
    if len(lengths) > MM.MAX_COUNT:
        raise PackError(E_RANGE, "more than 2^20 members")
    widths = [1] * len(lengths) if widths is None else list(widths)
    filters = [0] * len(lengths) if filters is None else list(filters)
    methods = [0] * len(lengths) if methods is None else list(methods)
    if (len(widths) != len(lengths) or len(filters) != len(lengths) or len(methods) != len(lengths) or any(ln == 0 for ln in lengths)
            or any(w not in MM.WIDTHS for w in widths) or any(f not in D.FILTERS + (AUTO,) for f in filters)
            or any(m not in M3.METHODS + (AUTO,) for m in methods)):
        raise PackError(E_ARG, "a zero length, a bad width, a bad filter or a bad method")
    if sum(lengths) > MAX_N:
        raise PackError(E_RANGE, "more than 2^32 bytes")
    return widths, filters, methods, sum(lengths)


@functools.lru_cache(maxsize=256)
def costs(member, w, f):
    """(chain cost, direct cost) of a member at width w under the filter f (0 or 1): stream bytes + 8 x extension-table words."""
    fm = D.encode(member, w).tobytes() if f else member
    chain = len(E.encode(Z.encode(P2.ranks(MM.split(fm, w).tobytes()))))
    segs = M3.direct_segments(fm, w)
    direct = sum(len(s) for s in E.encode_segments(b"".join(segs), [len(s) for s in segs]))
    return chain, direct + 8 * M3.table_words(len(member), w, ORDER0)


def choose_method(chain_cost, direct_cost):
    return ORDER0 if direct_cost < chain_cost else CHAIN


def resolve(members, widths=None, filters=AUTO, methods=AUTO):
    """The filters and methods the writer names, two lists; filters and methods: a scalar for all members or a list, AUTO among them."""
    members = [bytes(m) for m in members]
    filters = [filters] * len(members) if isinstance(filters, int) else filters
    methods = [methods] * len(members) if isinstance(methods, int) else methods
    widths, filters, methods, _ = check_args([len(m) for m in members], widths, filters, methods)
    fs = [EST.choose_filter(*EST.estimate(m, w)) if f == AUTO else f for m, w, f in zip(members, widths, filters)]
    ms = [choose_method(*costs(m, w, f)) if md == AUTO else md for m, w, f, md in zip(members, widths, fs, methods)]
    return fs, ms


def bound(lengths, widths=None, methods=AUTO):
    """bwts_pack_members_bound_a: the extension table with every AUTO member's words, an AUTO member's streams at the larger of its two
    bounds; 0 on bad arguments."""
    methods = [methods] * len(lengths) if isinstance(methods, int) and lengths is not None else methods
    try:
        widths, _, methods, _ = check_args(lengths, widths, None, methods)
    except PackError:
        return 0
    words = sum(M3.table_words(ln, w, ORDER0) for ln, w, m in zip(lengths, widths, methods) if m != CHAIN)
    total = M3.HEADER + M3.ENTRY * len(lengths) + 8 * (words + (words & 1))
    for ln, w, m in zip(lengths, widths, methods):
        chain, direct = E.bound(ln), sum(E.bound(s) for s in M3.segments(ln, w))
        total += chain if m == CHAIN else direct if m == ORDER0 else max(chain, direct)
    return total


def pack(members, widths=None, filters=AUTO, methods=AUTO):
    fs, ms = resolve(members, widths, filters, methods)
    return M3.pack(members, widths, fs, ms)
