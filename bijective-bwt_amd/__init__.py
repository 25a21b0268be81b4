"""Host-side Python mirror of the MI355X bijective-BWT engine.

Thin ctypes binding of the C-ABI in ``include/bwts.h`` (``libbwts_hip.so``).  The two
module-level functions keep the reference programs' meaning:

* :func:`mk_bwts`  -- forward BWTS of a byte string  (``/root/reference/mk_bwts_sa.c:33-65``)
* :func:`unbwts`   -- inverse BWTS of a byte string  (``/root/reference/unbwts.c:19-92``)

There is no CPU path here: if the HIP library is missing, or no GPU is usable, calls raise
:class:`BwtsError`.  (The CPU oracle lives under ``oracle/`` and is test infrastructure.)

The directory name contains a hyphen, so import it through ``load_package()`` of the
repo-root ``__graft_entry__`` or ``importlib`` (see ``tests/conftest.py``).
"""
import ctypes
import os
import re
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# BWTS_LIB_OVERRIDE: another build of the same library (A/B timing sessions on one GPU box, tools/sessions/*.sh); never set in tests
LIB_PATH = os.environ.get("BWTS_LIB_OVERRIDE") or os.path.join(PKG_DIR, "libbwts_hip.so")

KINDS = {"uniform256": 0, "zipf": 1, "dna": 2, "text": 3}

K_NAMES = ["histogram", "keybuild", "radix_hist", "radix_scan", "radix_scatter", "rerank", "lyndon", "emit",
           "lf_build", "walk", "listrank", "walk_emit", "other", "radix_scatter_main", "round"]
K_COUNT = len(K_NAMES)
MAX_ROUND_STATS = 40
H_NAMES = ["init", "module_load", "io_alloc", "staging_alloc", "arena_alloc"]
H_COUNT = len(H_NAMES)

# every symbol include/bwts.h declares (the drop-in surface) ...
EXPORTS = [
    "bwts_ctx_create", "bwts_ctx_destroy", "bwts_ctx_release_memory", "bwts_forward", "bwts_inverse", "bwts_forward_sink", "bwts_inverse_sink",
    "bwts_forward_device", "bwts_inverse_device", "bwts_last_timings", "bwts_kernel_class_name", "bwts_strerror",
    "bwts_last_hip_error", "bwts_set_timing", "bwts_host_alloc", "bwts_host_free", "bwts_host_cost_name",
    "bwts_forward_batch", "bwts_inverse_batch",
    "bwts_forward_segments", "bwts_inverse_segments", "bwts_forward_segments_device", "bwts_inverse_segments_device",
]
# ... include/bwts_mtf.h (move-to-front, the stage behind the transform) ...
MTF_EXPORTS = [
    "bwts_mtf_forward_device", "bwts_mtf_inverse_device", "bwts_mtf_forward", "bwts_mtf_inverse",
    "bwts_mtf_forward_segments_device", "bwts_mtf_inverse_segments_device", "bwts_mtf_forward_segments", "bwts_mtf_inverse_segments",
]
# ... include/bwts_ec.h (entropy coding of the ranks, the stage behind move-to-front) ...
EC_EXPORTS = [
    "bwts_ec_bound", "bwts_ec_bound_segments", "bwts_ec_decoded_size", "bwts_ec_encode_device", "bwts_ec_decode_device",
    "bwts_ec_encode", "bwts_ec_decode", "bwts_ec_encode_segments_device", "bwts_ec_decode_segments_device",
]
E_FORMAT, E_SPACE = -8, -9
# ... include/bwts_zrl.h (zero-run coding of the ranks, between move-to-front and the entropy coder) ...
ZRL_EXPORTS = [
    "bwts_zrl_bound", "bwts_zrl_encode_device", "bwts_zrl_decode_device", "bwts_zrl_encode", "bwts_zrl_decode",
    "bwts_zrl_encode_segments_device", "bwts_zrl_decode_segments_device",
]
# ... include/bwts_planes.h (byte-plane split of typed arrays, the stage in front of the transform) ...
PLANES_EXPORTS = [
    "bwts_planes_split_device", "bwts_planes_join_device", "bwts_planes_split_segments_device", "bwts_planes_join_segments_device",
    "bwts_planes_split", "bwts_planes_join",
]
# ... include/bwts_pack.h (the chain as one call: a checksummed frame) ...
PACK_EXPORTS = [
    "bwts_crc32_device", "bwts_crc32_segments_device", "bwts_pack_bound", "bwts_unpack_size",
    "bwts_pack_device", "bwts_unpack_device", "bwts_pack", "bwts_unpack",
    "bwts_pack_bound_v", "bwts_pack_device_v", "bwts_pack_v",
    "bwts_pack_planes_bound", "bwts_pack_planes_device", "bwts_pack_planes",
    "bwts_unpack_ranges_device", "bwts_unpack_ranges",
]
E_CHECKSUM = -10
# ... include/bwts_members.h (the member frame: arrays of any lengths and widths in one frame) ...
MEMBERS_EXPORTS = [
    "bwts_planes_split_segments_w_device", "bwts_planes_join_segments_w_device", "bwts_pack_members_bound",
    "bwts_pack_members_device", "bwts_pack_members", "bwts_frame_members", "bwts_unpack_members_device", "bwts_unpack_members",
    "bwts_pack_members_f_device", "bwts_pack_members_f", "bwts_frame_members_f",
    "bwts_pack_members_bound_m", "bwts_pack_members_m_device", "bwts_pack_members_m", "bwts_frame_members_m",
    "bwts_members_estimate_device", "bwts_members_estimate", "bwts_pack_members_bound_a", "bwts_pack_members_a_device", "bwts_pack_members_a",
    "bwts_gather_device", "bwts_scatter_device", "bwts_pack_members_p_device", "bwts_unpack_members_p_device",
]
# ... include/bwts_delta.h (delta filter of integer arrays, the stage in front of the byte-plane split) ...
DELTA_EXPORTS = [
    "bwts_delta_encode_device", "bwts_delta_decode_device", "bwts_delta_encode_segments_f_device", "bwts_delta_decode_segments_f_device",
    "bwts_delta_encode", "bwts_delta_decode",
]
FILTER_NONE, FILTER_DELTA = 0, 1
METHOD_CHAIN, METHOD_ORDER0 = 0, 1      # a member's method (member frame version 3): the whole chain, or its planes coded directly
FILTER_AUTO = METHOD_AUTO = 255         # pack_members_auto alone: the pack chooses (include/bwts_members.h, "AUTO")
# ... and include/bwts_test.h (harness and unit-test hooks)
TEST_EXPORTS = [
    "bwts_generate_device", "bwts_device_alloc", "bwts_device_free", "bwts_copy_to_device", "bwts_copy_to_host",
    "bwts_device_equal", "bwts_debug_sort_pairs", "bwts_debug_suffix_array", "bwts_debug_lyndon",
    "bwts_debug_chunk_plan", "bwts_debug_chunk_plan_target", "bwts_debug_inverse_arena", "bwts_debug_forward_arena", "bwts_debug_wide_forward_arena", "bwts_debug_inverse_report",
    "bwts_debug_forward_report", "bwts_debug_segments_plan", "bwts_debug_segments_report",
    "bwts_debug_mtf_plan", "bwts_debug_last_spans", "bwts_debug_ec_plan", "bwts_debug_crc_plan",
    "bwts_debug_zrl_plan", "bwts_debug_planes_plan", "bwts_debug_key_plan",
    "bwts_debug_unpack_ranges_plan", "bwts_debug_unpack_ranges_report", "bwts_debug_copy_pieces", "bwts_debug_rank_steps",
]
# bwts_debug_unpack_ranges_report: the words of the record, and the stages by their bits
RANGES_REPORT_FIELDS = ["blocks", "runs", "covered_bytes", "stream_bytes", "gathered", "pieces", "stages", "single"]
RANGES_STAGES = {1: "gather", 2: "decode", 4: "zrl", 8: "mtf", 16: "inverse", 32: "join", 64: "crc", 128: "cut", 256: "delta", 512: "regroup"}
# bwts_debug_inverse_report: the words of one attempt's record, and what marks, outcomes and forms are called
INV_REPORT_FIELDS = ["g", "mark", "outcome", "s", "virtual", "node_cap", "nu", "nu2", "ucap_first", "second_collect",
                     "listed_classes", "mom_fallback", "unit_rank", "kc", "kt", "form"]
INV_MARKS = {0: "log", 1: "sentinel", 2: "bytemap", 3: "moments"}
INV_OUTCOMES = {0: "DONE", 1: "RETRY_DENSE", 2: "AMBIGUOUS", 3: "NEED_LOG", 255: "ERROR"}
INV_FORMS = {0: "narrow", 1: "wide", 2: "wide_compact", 3: "segmented"}
# bwts_debug_segments_plan / bwts_debug_segments_report: the plans by name ("shared_nomem": the shared plan was refused for memory and
# the lane plan ran), and the route the plan's own segments take
SEG_PLANS = {0: "lane", 1: "shared", 2: "shared_nomem"}
# bwts_debug_forward_report: the header words of one sort's record (chunk words from 24 on), the words of a round's record by
# form, and what forms, reasons and ends are called
FWD_HEADER_WORDS, FWD_ROUND_WORDS = 48, 12
FWD_SORT_WORDS = FWD_HEADER_WORDS + MAX_ROUND_STATS * FWD_ROUND_WORDS
FWD_HEADER_FIELDS = ["cyclic", "n", "k", "sigma", "bits", "msym", "key_bits", "varlen", "hstep", "keys", "flags_outside_rank", "tied0",
                     "rank_early", "form", "no_chunks", "need_sa", "end", "rest_chunks", "rest_big", "rest_tiles", "rounds", "directory",
                     "order_sort", "left"]
FWD_DIRECT_WORD = 36            # header word: what became of the direct form
FWD_DIRECT = {0: "not_tried", 1: "settled", 2: "fallback_group", 3: "fallback_depth"}
FWD_LEAN_WORD = 37              # header word: what became of round 0's lean last pass (flags and tied positions, no sorted keys)
FWD_LEAN = {0: "not_tried", 1: "held", 2: "gave_up_seam", 3: "gave_up_count", 4: "gave_up_direct"}
FWD_CHUNK_FIELDS = ["S", "maxchunks", "a_small", "big0", "m_exit", "m_stay", "groups", "wide_possible", "fsl", "compactions",
                    "compactions_skipped", "enqueued_behind_last"]
# Later additions live beside the dicts above, whose keys are compared whole by the exact tests: header word 38, the nominal chunk size
# after the last compaction (0 without one), is "chunk_S_recut"; word 11 of a chunk round, the nominal size as the round ran, goes to
# the list "chunk_round_S" (one entry per recorded round)
FWD_CHUNK_S_RECUT_WORD = 38
FWD_ROUND_CHUNK_S_WORD = 11
FWD_ROUND_FIELDS = {"sparse": ["form", "h", "in", "out", "splits", "probe", "m_big", "whole", "skip_next"],
                    "chunks": ["form", "h", "in", "out", "splits", "chunks_in", "chunks_out", "big_in", "big_stays", "big_leaves", "nchunks"],
                    "tiles": ["form", "h", "in", "out", "splits", "m_big"],
                    "direct": ["form", "h", "in", "out", "splits"]}
FWD_FORMS = {0: "none", 1: "sparse", 2: "chunks", 3: "tiles", 4: "direct"}
FWD_KEYS = {0: "wide", 1: "split32", 2: "split40"}
FWD_NO_CHUNKS = {0: None, 1: "short_list", 2: "knob", 3: "no_room_store", 4: "no_room_order", 5: "no_room_biglist"}
FWD_ENDS = {0: "none", 1: "empty", 2: "stable"}
FWD_PROBES = {0: "short_list", 1: "ran", 2: "skipped"}


class BwtsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("bwts error %d: %s" % (code, msg))
        self.code = code


class KernelStat(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double), ("launches", ctypes.c_uint64), ("elems", ctypes.c_uint64),
                ("alg_bytes", ctypes.c_uint64)]


class Timings(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double),
                ("n", ctypes.c_uint64), ("factors", ctypes.c_uint64), ("rounds", ctypes.c_uint32),
                ("lyndon_rounds", ctypes.c_uint32), ("key_symbols", ctypes.c_uint32), ("key_bits", ctypes.c_uint32),
                ("active_after_round0", ctypes.c_uint64), ("unvisited", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64),
                ("round_active", ctypes.c_uint64 * MAX_ROUND_STATS), ("k", KernelStat * K_COUNT),
                ("host_ms", ctypes.c_double * H_COUNT), ("attempts", ctypes.c_uint32), ("reserved_", ctypes.c_uint32)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_ if f not in ("k", "round_active", "host_ms")}
        d["host_ms"] = {H_NAMES[i]: float(self.host_ms[i]) for i in range(H_COUNT)}
        d["round_active"] = [int(v) for v in self.round_active[: max(int(self.rounds), 1)]]
        d["kernels"] = {K_NAMES[i]: {"ms": self.k[i].ms, "launches": self.k[i].launches, "elems": self.k[i].elems,
                                     "alg_bytes": self.k[i].alg_bytes} for i in range(K_COUNT) if self.k[i].launches}
        return d


SINK_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)

_lib = None


def build(verbose=False):
    """Compile libbwts_hip.so (gfx950) and the CLIs in-tree with hipcc."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", PKG_DIR, "-j4", "all"], stdout=out)


def lib():
    """The loaded C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BwtsError(-2, "libbwts_hip.so is not built (run `make -C bijective-bwt_amd` or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.bwts_ctx_create.argtypes = [ctypes.POINTER(vp), i32]
        L.bwts_ctx_destroy.argtypes = [vp]
        L.bwts_ctx_destroy.restype = None
        L.bwts_ctx_release_memory.argtypes = [vp]
        L.bwts_ctx_release_memory.restype = ctypes.c_int
        for name in ("bwts_forward", "bwts_inverse", "bwts_forward_device", "bwts_inverse_device"):
            getattr(L, name).argtypes = [vp, vp, u64, vp]
        L.bwts_last_timings.argtypes = [vp, ctypes.POINTER(Timings)]
        L.bwts_kernel_class_name.argtypes = [i32]
        L.bwts_kernel_class_name.restype = ctypes.c_char_p
        L.bwts_strerror.argtypes = [i32]
        L.bwts_strerror.restype = ctypes.c_char_p
        L.bwts_last_hip_error.argtypes = [vp]
        L.bwts_set_timing.argtypes = [vp, i32]
        L.bwts_host_alloc.argtypes = [vp, u64, ctypes.POINTER(vp)]
        L.bwts_host_free.argtypes = [vp, vp]
        for name in ("bwts_forward_batch", "bwts_inverse_batch"):
            getattr(L, name).argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(u64), ctypes.POINTER(vp)]
        for name in ("bwts_forward_segments", "bwts_inverse_segments", "bwts_forward_segments_device", "bwts_inverse_segments_device"):
            getattr(L, name).argtypes = [vp, vp, vp, u64, vp]
        for name in ("bwts_mtf_forward", "bwts_mtf_inverse", "bwts_mtf_forward_device", "bwts_mtf_inverse_device"):
            getattr(L, name).argtypes = [vp, vp, u64, vp]
        for name in ("bwts_mtf_forward_segments", "bwts_mtf_inverse_segments", "bwts_mtf_forward_segments_device", "bwts_mtf_inverse_segments_device"):
            getattr(L, name).argtypes = [vp, vp, vp, u64, vp]
        L.bwts_debug_mtf_plan.argtypes = [u64, ctypes.POINTER(u64)]
        L.bwts_debug_last_spans.argtypes = [vp, ctypes.POINTER(ctypes.c_double), u64]
        L.bwts_ec_bound.argtypes = [u64]
        L.bwts_ec_bound.restype = u64
        L.bwts_ec_bound_segments.argtypes = [vp, u64, ctypes.POINTER(u64)]
        L.bwts_ec_decoded_size.argtypes = [vp, u64, ctypes.POINTER(u64)]
        for name in ("bwts_ec_encode_device", "bwts_ec_decode_device", "bwts_ec_encode", "bwts_ec_decode"):
            getattr(L, name).argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_ec_encode_segments_device.argtypes = [vp, vp, vp, u64, vp, u64, vp]
        L.bwts_ec_decode_segments_device.argtypes = [vp, vp, vp, vp, u64, vp]
        L.bwts_debug_ec_plan.argtypes = [u64, ctypes.POINTER(u64)]
        L.bwts_zrl_bound.argtypes = [u64]
        L.bwts_zrl_bound.restype = u64
        for name in ("bwts_zrl_encode_device", "bwts_zrl_encode"):
            getattr(L, name).argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        for name in ("bwts_zrl_decode_device", "bwts_zrl_decode"):
            getattr(L, name).argtypes = [vp, vp, u64, vp, u64]
        L.bwts_zrl_encode_segments_device.argtypes = [vp, vp, vp, u64, vp, u64, vp]
        L.bwts_zrl_decode_segments_device.argtypes = [vp, vp, vp, vp, u64, vp]
        L.bwts_debug_zrl_plan.argtypes = [u64, ctypes.POINTER(u64)]
        u32 = ctypes.c_uint32
        for name in ("bwts_planes_split_device", "bwts_planes_join_device", "bwts_planes_split", "bwts_planes_join"):
            getattr(L, name).argtypes = [vp, vp, u64, u32, vp]
        for name in ("bwts_planes_split_segments_device", "bwts_planes_join_segments_device"):
            getattr(L, name).argtypes = [vp, vp, vp, u64, u32, vp]
        L.bwts_debug_planes_plan.argtypes = [u64, u32, ctypes.POINTER(u64)]
        L.bwts_crc32_device.argtypes = [vp, vp, u64, ctypes.POINTER(ctypes.c_uint32)]
        L.bwts_crc32_segments_device.argtypes = [vp, vp, vp, u64, vp]
        L.bwts_pack_bound.argtypes = [u64, u64]
        L.bwts_pack_bound.restype = u64
        L.bwts_unpack_size.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        for name in ("bwts_pack_device", "bwts_pack"):
            getattr(L, name).argtypes = [vp, vp, u64, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_pack_bound_v.argtypes = [u32, u64, u64]
        L.bwts_pack_bound_v.restype = u64
        for name in ("bwts_pack_device_v", "bwts_pack_v"):
            getattr(L, name).argtypes = [vp, u32, vp, u64, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_pack_planes_bound.argtypes = [u32, u64, u64]
        L.bwts_pack_planes_bound.restype = u64
        for name in ("bwts_pack_planes_device", "bwts_pack_planes"):
            getattr(L, name).argtypes = [vp, u32, vp, u64, u64, vp, u64, ctypes.POINTER(u64)]
        for name in ("bwts_unpack_device", "bwts_unpack"):
            getattr(L, name).argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_debug_crc_plan.argtypes = [u64, ctypes.POINTER(u64)]
        for name in ("bwts_unpack_ranges_device", "bwts_unpack_ranges"):
            getattr(L, name).argtypes = [vp, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_debug_unpack_ranges_plan.argtypes = [vp, u64, vp, u64, u64, ctypes.POINTER(u64), vp, u64]
        L.bwts_debug_unpack_ranges_report.argtypes = [vp, ctypes.POINTER(u64)]
        L.bwts_debug_copy_pieces.argtypes = [vp, vp, u64, vp, u64, vp, u64]
        for name in ("bwts_planes_split_segments_w_device", "bwts_planes_join_segments_w_device"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, u64, vp]
        L.bwts_pack_members_bound.argtypes = [vp, u64]
        L.bwts_pack_members_bound.restype = u64
        for name in ("bwts_pack_members_device", "bwts_pack_members"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_frame_members.argtypes = [vp, u64, vp, vp, u64, ctypes.POINTER(u64)]
        for name in ("bwts_unpack_members_device", "bwts_unpack_members"):
            getattr(L, name).argtypes = [vp, vp, u64, vp, u64, vp, u64, ctypes.POINTER(u64)]
        for name in ("bwts_pack_members_f_device", "bwts_pack_members_f"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_frame_members_f.argtypes = [vp, u64, vp, vp, vp, u64, ctypes.POINTER(u64)]
        L.bwts_pack_members_bound_m.argtypes = [vp, vp, vp, u64]
        L.bwts_pack_members_bound_m.restype = u64
        for name in ("bwts_pack_members_m_device", "bwts_pack_members_m"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_frame_members_m.argtypes = [vp, u64, vp, vp, vp, vp, u64, ctypes.POINTER(u64)]
        for name in ("bwts_members_estimate_device", "bwts_members_estimate"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, u64, vp, vp]
        L.bwts_pack_members_bound_a.argtypes = [vp, vp, vp, u64]
        L.bwts_pack_members_bound_a.restype = u64
        for name in ("bwts_pack_members_a_device", "bwts_pack_members_a"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, u64, ctypes.POINTER(u64), vp, vp]
        L.bwts_gather_device.argtypes = [vp, vp, vp, u64, vp]
        L.bwts_scatter_device.argtypes = [vp, vp, vp, vp, u64]
        L.bwts_pack_members_p_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, u64, ctypes.POINTER(u64), vp, vp]
        L.bwts_unpack_members_p_device.argtypes = [vp, vp, u64, vp, u64, vp, vp]
        for name in ("bwts_delta_encode_device", "bwts_delta_decode_device", "bwts_delta_encode", "bwts_delta_decode"):
            getattr(L, name).argtypes = [vp, vp, u64, u32, vp]
        for name in ("bwts_delta_encode_segments_f_device", "bwts_delta_decode_segments_f_device"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, vp, u64, vp]
        for name in ("bwts_forward_sink", "bwts_inverse_sink"):
            getattr(L, name).argtypes = [vp, vp, u64, SINK_FN, vp]
        L.bwts_generate_device.argtypes = [vp, i32, u64, u64, vp]
        L.bwts_device_alloc.argtypes = [vp, u64, ctypes.POINTER(vp)]
        L.bwts_device_free.argtypes = [vp, vp]
        L.bwts_copy_to_device.argtypes = [vp, vp, vp, u64]
        L.bwts_copy_to_host.argtypes = [vp, vp, vp, u64]
        L.bwts_device_equal.argtypes = [vp, vp, vp, u64, ctypes.POINTER(i32)]
        L.bwts_debug_sort_pairs.argtypes = [vp, vp, vp, u64, i32]
        L.bwts_debug_rank_steps.argtypes = [vp, vp, vp, i32, vp, vp]
        L.bwts_debug_suffix_array.argtypes = [vp, vp, u64, vp]
        L.bwts_debug_lyndon.argtypes = [vp, vp, u64, vp, u64, ctypes.POINTER(u64)]
        L.bwts_debug_chunk_plan.argtypes = [u64, u64, ctypes.POINTER(u64)]
        L.bwts_debug_chunk_plan_target.argtypes = [u64, u64, ctypes.c_uint32, ctypes.POINTER(u64)]
        L.bwts_debug_key_plan.argtypes = [vp, u64, i32, i32, i32, i32, i32, vp, ctypes.POINTER(u64), vp, vp]
        L.bwts_debug_inverse_arena.argtypes = [u64, i32, i32, ctypes.POINTER(u64)]
        L.bwts_debug_forward_arena.argtypes = [u64, ctypes.POINTER(u64)]
        L.bwts_debug_wide_forward_arena.argtypes = [u64, i32, i32, u64, ctypes.POINTER(u64)]
        L.bwts_debug_inverse_report.argtypes = [vp, ctypes.POINTER(u64), u64, ctypes.POINTER(u64)]
        L.bwts_debug_forward_report.argtypes = [vp, ctypes.POINTER(u64), u64, ctypes.POINTER(u64)]
        L.bwts_debug_segments_plan.argtypes = [vp, u64, ctypes.POINTER(u64)]
        L.bwts_debug_segments_report.argtypes = [vp, ctypes.POINTER(u64)]
        _lib = L
    return _lib


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


class DeviceBuffer:
    """A raw device allocation owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = ctypes.c_void_p()
        ctx._check(lib().bwts_device_alloc(ctx._h, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            lib().bwts_device_free(self.ctx._h, self.ptr)
            self.ptr = None

    def upload(self, data):
        a = _u8(data)
        assert a.size <= self.nbytes
        self.ctx._check(lib().bwts_copy_to_device(self.ctx._h, self.ptr, a.ctypes.data, a.size))

    def download(self, nbytes=None):
        n = self.nbytes if nbytes is None else int(nbytes)
        out = np.empty(n, dtype=np.uint8)
        self.ctx._check(lib().bwts_copy_to_host(self.ctx._h, out.ctypes.data, self.ptr, n))
        return out


class Context:
    """One GPU context (``bwts_ctx``): owns a stream, a device arena and pinned staging."""

    def __init__(self, device=0):
        self._h = None
        h = ctypes.c_void_p()
        rc = lib().bwts_ctx_create(ctypes.byref(h), int(device))
        if rc != 0:
            raise BwtsError(rc, lib().bwts_strerror(rc).decode())
        self._h = h
        self.device = int(device)

    def close(self):
        if self._h:
            lib().bwts_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_memory(self):
        """Hands the device memory the context keeps between calls back to the device (bwts_ctx_release_memory)."""
        self._check(lib().bwts_ctx_release_memory(self._h))

    def _check(self, rc):
        if rc != 0:
            msg = lib().bwts_strerror(rc).decode()
            if rc == -4:
                msg += " (hipError %d)" % lib().bwts_last_hip_error(self._h)
            raise BwtsError(rc, msg)

    # -- host-buffer transforms ------------------------------------------------------
    def _host(self, fn, data):
        a = _u8(data)
        if a.size == 0:
            raise BwtsError(-1, "empty input (the reference fails on empty files: map_file.c:36-40)")
        out = np.empty_like(a)
        self._check(fn(self._h, a.ctypes.data, a.size, out.ctypes.data))
        return out

    def forward(self, data):
        return self._host(lib().bwts_forward, data)

    def inverse(self, data):
        return self._host(lib().bwts_inverse, data)

    # -- device-buffer transforms ------------------------------------------------------
    def forward_device(self, d_in, n, d_out):
        self._check(lib().bwts_forward_device(self._h, _ptr(d_in), int(n), _ptr(d_out)))

    def inverse_device(self, d_in, n, d_out):
        self._check(lib().bwts_inverse_device(self._h, _ptr(d_in), int(n), _ptr(d_out)))

    def set_timing(self, level=2):
        """HIP-event times in timings(): 0 off (default), 1 dominant kernels only, 2 every class (~1 ms per call at 1 GiB)."""
        self._check(lib().bwts_set_timing(self._h, int(level)))

    def _sink(self, fn, data):
        a = _u8(data)
        pieces = []

        def take(_user, ptr, length):
            pieces.append(ctypes.string_at(ptr, length))
            return 0

        cb = SINK_FN(take)
        self._check(fn(self._h, a.ctypes.data, a.size, cb, None))
        return np.frombuffer(b"".join(pieces), dtype=np.uint8)

    def forward_sink(self, data):
        """forward() with the output delivered through the sink callback (what the CLIs use)."""
        return self._sink(lib().bwts_forward_sink, data)

    def inverse_sink(self, data):
        return self._sink(lib().bwts_inverse_sink, data)

    def host_alloc(self, nbytes):
        """A pinned host block as a numpy uint8 array (freed with the context or host_free())."""
        p = ctypes.c_void_p()
        self._check(lib().bwts_host_alloc(self._h, int(nbytes), ctypes.byref(p)))
        arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(int(nbytes),))
        return arr, p.value

    def host_free(self, ptr):
        self._check(lib().bwts_host_free(self._h, ptr))

    def _batch(self, fn, arrays):
        arrs = [_u8(a) for a in arrays]
        outs = [np.empty_like(a) for a in arrs]
        k = len(arrs)
        ins_p = (ctypes.c_void_p * k)(*[a.ctypes.data for a in arrs])
        outs_p = (ctypes.c_void_p * k)(*[o.ctypes.data for o in outs])
        ns = (ctypes.c_uint64 * k)(*[a.size for a in arrs])
        self._check(fn(self._h, k, ins_p, ns, outs_p))
        return outs

    def forward_batch(self, arrays):
        """bwts_forward_batch: the transforms of several inputs, copies overlapped with the neighbours' transforms."""
        return self._batch(lib().bwts_forward_batch, arrays)

    def inverse_batch(self, arrays):
        return self._batch(lib().bwts_inverse_batch, arrays)

    # -- independent segments in one device pass -----------------------------------------
    def _segments(self, fn, data, lengths, out=None):
        a = _u8(data)
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        if int(ls.sum(dtype=np.uint64)) != a.size or (ls.size and int(ls.max()) > a.size):
            raise BwtsError(-1, "segment lengths do not add up to the input's size")
        if out is None:
            out = np.empty_like(a)
        elif out.size < a.size:
            raise BwtsError(-1, "output smaller than the input")
        self._check(fn(self._h, a.ctypes.data, ls.ctypes.data, ls.size, out.ctypes.data))
        return out

    def forward_segments(self, data, lengths, out=None):
        """bwts_forward_segments: data holds len(lengths) consecutive segments; each is transformed on its own, in one device pass.
        `out` (optional) is a caller-provided uint8 array, which may be `data` itself."""
        return self._segments(lib().bwts_forward_segments, data, lengths, out)

    def inverse_segments(self, data, lengths, out=None):
        return self._segments(lib().bwts_inverse_segments, data, lengths, out)

    def forward_segments_device(self, d_in, lengths, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(lib().bwts_forward_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, _ptr(d_out)))

    def inverse_segments_device(self, d_in, lengths, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(lib().bwts_inverse_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, _ptr(d_out)))

    # -- move-to-front behind the transform (include/bwts_mtf.h) ------------------------------
    def mtf_forward(self, data):
        """bwts_mtf_forward: the move-to-front ranks of a byte string (host buffers, staged like forward())."""
        return self._host(lib().bwts_mtf_forward, data)

    def mtf_inverse(self, data):
        return self._host(lib().bwts_mtf_inverse, data)

    def mtf_forward_device(self, d_in, n, d_out):
        self._check(lib().bwts_mtf_forward_device(self._h, _ptr(d_in), int(n), _ptr(d_out)))

    def mtf_inverse_device(self, d_in, n, d_out):
        self._check(lib().bwts_mtf_inverse_device(self._h, _ptr(d_in), int(n), _ptr(d_out)))

    def mtf_forward_segments(self, data, lengths, out=None):
        """bwts_mtf_forward_segments: the list starts afresh at every segment; `out` may be `data` itself."""
        return self._segments(lib().bwts_mtf_forward_segments, data, lengths, out)

    def mtf_inverse_segments(self, data, lengths, out=None):
        return self._segments(lib().bwts_mtf_inverse_segments, data, lengths, out)

    def mtf_forward_segments_device(self, d_in, lengths, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(lib().bwts_mtf_forward_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, _ptr(d_out)))

    def mtf_inverse_segments_device(self, d_in, lengths, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(lib().bwts_mtf_inverse_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, _ptr(d_out)))

    # -- entropy coding behind move-to-front (include/bwts_ec.h) ------------------------------------
    def ec_encode(self, data, out_cap=None):
        """bwts_ec_encode: the rANS stream of a byte string (host buffers); out_cap defaults to the bound."""
        a = _u8(data)
        if a.size == 0:
            raise BwtsError(-1, "empty input")
        out = np.empty(ec_bound(a.size) if out_cap is None else int(out_cap), dtype=np.uint8)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_ec_encode(self._h, a.ctypes.data, a.size, out.ctypes.data, out.size, ctypes.byref(got)))
        return out[:got.value].copy()

    def ec_decode(self, stream):
        """bwts_ec_decode: the bytes a stream holds (host buffers); the output is sized from the stream's header."""
        a = _u8(stream)
        n = ec_decoded_size(a)
        out = np.empty(n, dtype=np.uint8)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_ec_decode(self._h, a.ctypes.data, a.size, out.ctypes.data, out.size, ctypes.byref(got)))
        return out[:got.value]

    def ec_encode_device(self, d_in, n, d_out, out_cap):
        """bwts_ec_encode_device: returns the stream's size in bytes."""
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_ec_encode_device(self._h, _ptr(d_in), int(n), _ptr(d_out), int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def ec_decode_device(self, d_in, in_bytes, d_out, out_cap):
        """bwts_ec_decode_device: returns the number of bytes decoded."""
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_ec_decode_device(self._h, _ptr(d_in), int(in_bytes), _ptr(d_out), int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def ec_encode_segments_device(self, d_in, lengths, d_out, out_cap):
        """bwts_ec_encode_segments_device: one stream per segment, concatenated; returns their sizes (uint64 array)."""
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        sizes = np.zeros(ls.size, dtype=np.uint64)
        self._check(lib().bwts_ec_encode_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, _ptr(d_out), int(out_cap), sizes.ctypes.data))
        return sizes

    def ec_decode_segments_device(self, d_in, stream_bytes, lengths, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        sb = np.ascontiguousarray(stream_bytes, dtype=np.uint64)
        if sb.size != ls.size:
            raise BwtsError(-1, "one stream size per segment")
        self._check(lib().bwts_ec_decode_segments_device(self._h, _ptr(d_in), sb.ctypes.data, ls.ctypes.data, ls.size, _ptr(d_out)))

    # -- zero-run coding between move-to-front and the entropy coder (include/bwts_zrl.h) -----------
    def zrl_encode(self, data, out_cap=None):
        """bwts_zrl_encode: the zero-run coded form of a byte string, or the string itself where that is no shorter (host buffers);
        out_cap defaults to the bound, the input's length."""
        a = _u8(data)
        if a.size == 0:
            raise BwtsError(-1, "empty input")
        out = np.empty(a.size if out_cap is None else int(out_cap), dtype=np.uint8)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_zrl_encode(self._h, a.ctypes.data, a.size, out.ctypes.data, out.size, ctypes.byref(got)))
        return out[:got.value].copy()

    def zrl_decode(self, coded, n):
        """bwts_zrl_decode: the n bytes a coded form stands for (host buffers)."""
        a = _u8(coded)
        out = np.empty(int(n), dtype=np.uint8)
        self._check(lib().bwts_zrl_decode(self._h, a.ctypes.data, a.size, out.ctypes.data, out.size))
        return out

    def zrl_encode_device(self, d_in, n, d_out, out_cap):
        """bwts_zrl_encode_device: returns the bytes written (below n: coded; n: stored)."""
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_zrl_encode_device(self._h, _ptr(d_in), int(n), _ptr(d_out), int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def zrl_decode_device(self, d_in, in_bytes, d_out, n):
        self._check(lib().bwts_zrl_decode_device(self._h, _ptr(d_in), int(in_bytes), _ptr(d_out), int(n)))

    def zrl_encode_segments_device(self, d_in, lengths, d_out, out_cap):
        """bwts_zrl_encode_segments_device: one output per segment, concatenated; returns their lengths (uint64 array)."""
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        sizes = np.zeros(ls.size, dtype=np.uint64)
        self._check(lib().bwts_zrl_encode_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, _ptr(d_out), int(out_cap), sizes.ctypes.data))
        return sizes

    def zrl_decode_segments_device(self, d_in, in_lengths, lengths, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        il = np.ascontiguousarray(in_lengths, dtype=np.uint64)
        if il.size != ls.size:
            raise BwtsError(-1, "one coded length per segment")
        self._check(lib().bwts_zrl_decode_segments_device(self._h, _ptr(d_in), il.ctypes.data, ls.ctypes.data, ls.size, _ptr(d_out)))

    # -- byte-plane split in front of the transform (include/bwts_planes.h) -------------------------------
    def _planes_host(self, fn, data, width):
        a = _u8(data)
        if a.size == 0:
            raise BwtsError(-1, "empty input")
        out = np.empty_like(a)
        self._check(fn(self._h, a.ctypes.data, a.size, int(width), out.ctypes.data))
        return out

    def planes_split(self, data, width):
        """bwts_planes_split: byte k of every `width`-byte element gathered into plane k, the tail copied (host buffers)."""
        return self._planes_host(lib().bwts_planes_split, data, width)

    def planes_join(self, data, width):
        """bwts_planes_join: the inverse of planes_split (host buffers)."""
        return self._planes_host(lib().bwts_planes_join, data, width)

    def planes_split_device(self, d_in, n, width, d_out):
        self._check(lib().bwts_planes_split_device(self._h, _ptr(d_in), int(n), int(width), _ptr(d_out)))

    def planes_join_device(self, d_in, n, width, d_out):
        self._check(lib().bwts_planes_join_device(self._h, _ptr(d_in), int(n), int(width), _ptr(d_out)))

    def planes_split_segments_device(self, d_in, lengths, width, d_out):
        """bwts_planes_split_segments_device: every segment split on its own, where it lies."""
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(lib().bwts_planes_split_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, int(width), _ptr(d_out)))

    def planes_join_segments_device(self, d_in, lengths, width, d_out):
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        self._check(lib().bwts_planes_join_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, int(width), _ptr(d_out)))

    # -- delta filter in front of the byte-plane split (include/bwts_delta.h) -------------------------------
    def delta_encode(self, data, width):
        """bwts_delta_encode: every `width`-byte element replaced by the zigzag of its difference to the one before, the tail copied
        (host buffers)."""
        return self._planes_host(lib().bwts_delta_encode, data, width)

    def delta_decode(self, data, width):
        """bwts_delta_decode: the inverse of delta_encode (host buffers)."""
        return self._planes_host(lib().bwts_delta_decode, data, width)

    def delta_encode_device(self, d_in, n, width, d_out):
        self._check(lib().bwts_delta_encode_device(self._h, _ptr(d_in), int(n), int(width), _ptr(d_out)))

    def delta_decode_device(self, d_in, n, width, d_out):
        self._check(lib().bwts_delta_decode_device(self._h, _ptr(d_in), int(n), int(width), _ptr(d_out)))

    def delta_encode_segments_f_device(self, d_in, lengths, widths, filters, d_out):
        """bwts_delta_encode_segments_f_device: every segment at its own width, encoded (filter 1) or copied (filter 0), where it lies."""
        ls, ws, fs = _members_f(lengths, widths, filters)
        self._check(lib().bwts_delta_encode_segments_f_device(self._h, _ptr(d_in), ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ls.size, _ptr(d_out)))

    def delta_decode_segments_f_device(self, d_in, lengths, widths, filters, d_out):
        ls, ws, fs = _members_f(lengths, widths, filters)
        self._check(lib().bwts_delta_decode_segments_f_device(self._h, _ptr(d_in), ls.ctypes.data, ws.ctypes.data, fs.ctypes.data, ls.size, _ptr(d_out)))

    # -- the chain as one call: a checksummed frame (include/bwts_pack.h) -----------------------------
    def crc32_device(self, d_in, n):
        """bwts_crc32_device: zlib's CRC-32 of n device bytes."""
        got = ctypes.c_uint32(0)
        self._check(lib().bwts_crc32_device(self._h, _ptr(d_in), int(n), ctypes.byref(got)))
        return int(got.value)

    def crc32_segments_device(self, d_in, lengths):
        """bwts_crc32_segments_device: one CRC-32 per segment (uint32 array)."""
        ls = np.ascontiguousarray(lengths, dtype=np.uint64)
        crcs = np.zeros(ls.size, dtype=np.uint32)
        self._check(lib().bwts_crc32_segments_device(self._h, _ptr(d_in), ls.ctypes.data, ls.size, crcs.ctypes.data))
        return crcs

    def pack(self, data, block_bytes=0, out_cap=None, version=None, planes=None):
        """bwts_pack_v: the frame of a byte string (host buffers); out_cap defaults to the bound; version 2: zero-run coding in front
        of the coder.  planes=2, 4 or 8 (bwts_pack_planes): a frame of version 3, the byte-plane split at that width in front of the
        transform."""
        a = _u8(data)
        if a.size == 0:
            raise BwtsError(-1, "empty input")
        version = _pack_version(version, planes)
        out = np.empty(pack_bound(a.size, block_bytes, version, planes) if out_cap is None else int(out_cap), dtype=np.uint8)
        got = ctypes.c_uint64(0)
        if planes is None:
            self._check(lib().bwts_pack_v(self._h, version, a.ctypes.data, a.size, int(block_bytes), out.ctypes.data, out.size, ctypes.byref(got)))
        else:
            self._check(lib().bwts_pack_planes(self._h, int(planes), a.ctypes.data, a.size, int(block_bytes), out.ctypes.data, out.size, ctypes.byref(got)))
        return out[:got.value].copy()

    def unpack(self, frame, out=None):
        """bwts_unpack: the bytes a frame holds (host buffers); the output is sized from the frame's header unless `out` is given."""
        a = _u8(frame)
        if out is None:
            out = np.empty(unpack_size(a)[0], dtype=np.uint8)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_unpack(self._h, a.ctypes.data, a.size, out.ctypes.data, out.size, ctypes.byref(got)))
        return out[:got.value]

    def pack_device(self, d_in, n, block_bytes, d_out, out_cap, version=None, planes=None):
        """bwts_pack_device_v, or with planes=2, 4 or 8 bwts_pack_planes_device (version 3): returns the frame's size in bytes."""
        got = ctypes.c_uint64(0)
        version = _pack_version(version, planes)
        if planes is None:
            self._check(lib().bwts_pack_device_v(self._h, version, _ptr(d_in), int(n), int(block_bytes), _ptr(d_out), int(out_cap), ctypes.byref(got)))
        else:
            self._check(lib().bwts_pack_planes_device(self._h, int(planes), _ptr(d_in), int(n), int(block_bytes), _ptr(d_out), int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def unpack_device(self, d_in, in_bytes, d_out, out_cap):
        """bwts_unpack_device: returns the number of bytes unpacked."""
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_unpack_device(self._h, _ptr(d_in), int(in_bytes), _ptr(d_out), int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def unpack_ranges(self, frame, ranges):
        """bwts_unpack_ranges: the bytes of every (offset, nbytes) range of the unpacked input, one uint8 array per range, in the
        order given (host buffers).  Only the blocks the ranges touch are decoded, and only their checksums are held against the
        frame's: damage in a block no range touches goes unnoticed."""
        a, rs = _u8(frame), _ranges(ranges)
        total = sum(int(b) for _, b in rs.tolist())
        out = np.empty(max(total, 1), dtype=np.uint8)[:total]       # (never a null pointer: the library judges the ranges itself)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_unpack_ranges(self._h, a.ctypes.data, a.size, rs.ctypes.data if rs.size else None, len(rs), out.ctypes.data, total,
                                             ctypes.byref(got)))
        ends = np.cumsum(rs[:, 1], dtype=np.uint64).tolist()
        return [out[e - int(b):e] for e, b in zip(ends, rs[:, 1].tolist())]

    def unpack_range(self, frame, offset, nbytes):
        """unpack_ranges with one range."""
        return self.unpack_ranges(frame, [(offset, nbytes)])[0]

    def unpack_ranges_device(self, d_in, in_bytes, ranges, d_out, out_cap):
        """bwts_unpack_ranges_device: the ranges' bytes back to back in d_out; returns their sum."""
        rs = _ranges(ranges)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_unpack_ranges_device(self._h, _ptr(d_in), int(in_bytes), rs.ctypes.data if rs.size else None, len(rs), _ptr(d_out),
                                                    int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def debug_unpack_ranges_report(self):
        """What the most recent unpack_ranges / unpack_ranges_device on this context did (RANGES_REPORT_FIELDS; "stages": the names
        of the stages that ran, "stage_bits": the word itself; "gathered" and "single" as bool)."""
        buf = (ctypes.c_uint64 * 8)()
        self._check(lib().bwts_debug_unpack_ranges_report(self._h, buf))
        d = {f: int(buf[i]) for i, f in enumerate(RANGES_REPORT_FIELDS)}
        d["stage_bits"], d["stages"] = d["stages"], [name for bit, name in RANGES_STAGES.items() if d["stages"] & bit]
        d["gathered"], d["single"] = bool(d["gathered"]), bool(d["single"])
        return d

    # -- the member frame: arrays of any lengths and widths in one frame (include/bwts_members.h) ---------
    def planes_split_segments_w_device(self, d_in, lengths, widths, d_out):
        """bwts_planes_split_segments_w_device: every segment split at its own width (1: copied), where it lies, in one launch."""
        ls, ws = _members(lengths, widths)
        self._check(lib().bwts_planes_split_segments_w_device(self._h, _ptr(d_in), ls.ctypes.data, ws.ctypes.data, ls.size, _ptr(d_out)))

    def planes_join_segments_w_device(self, d_in, lengths, widths, d_out):
        ls, ws = _members(lengths, widths)
        self._check(lib().bwts_planes_join_segments_w_device(self._h, _ptr(d_in), ls.ctypes.data, ws.ctypes.data, ls.size, _ptr(d_out)))

    def pack_members(self, arrays, widths=None, filters=None, out_cap=None, methods=None):
        """bwts_pack_members_m: one member frame of the arrays (bytes-like, or numpy arrays of any dtype, taken as their bytes); widths: one
        of 1, 2, 4, 8 per array, None for no split at all; filters: 0 or 1 (FILTER_DELTA: the delta filter of include/bwts_delta.h at the
        array's width) per array, None for none; methods: 0 or 1 (METHOD_ORDER0: the array's byte planes coded directly, for weights,
        noise and hashes) per array, None for the whole chain everywhere -- all named by the caller, never guessed from a dtype (host
        buffers)."""
        parts = [_bytes_of(a) for a in arrays]
        ls, ws = _members([p.size for p in parts], widths)
        fs, ms = _filters(ls, filters), _methods(ls, methods)
        a = np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)
        out = np.empty(pack_members_bound(ls, ws, ms) if out_cap is None else int(out_cap), dtype=np.uint8)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_pack_members_m(self._h, a.ctypes.data, ls.ctypes.data, None if ws is None else ws.ctypes.data,
                                              None if fs is None else fs.ctypes.data, None if ms is None else ms.ctypes.data, ls.size,
                                              out.ctypes.data, out.size, ctypes.byref(got)))
        return out[:got.value].copy()

    def pack_members_device(self, d_in, lengths, widths, d_out, out_cap, filters=None, methods=None):
        """bwts_pack_members_m_device: the members lie back to back in d_in; returns the frame's size in bytes."""
        ls, ws = _members(lengths, widths)
        fs, ms = _filters(ls, filters), _methods(ls, methods)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_pack_members_m_device(self._h, _ptr(d_in), ls.ctypes.data, None if ws is None else ws.ctypes.data,
                                                     None if fs is None else fs.ctypes.data, None if ms is None else ms.ctypes.data, ls.size,
                                                     _ptr(d_out), int(out_cap), ctypes.byref(got)))
        return int(got.value)

    def members_estimate(self, arrays, widths=None):
        """bwts_members_estimate: what the order-0 coder would make of every array's byte planes without a filter and with the delta
        filter, two lists of bytes (host buffers); widths as in pack_members."""
        parts = [_bytes_of(a) for a in arrays]
        ls, ws = _members([p.size for p in parts], widths)
        a = np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)
        e0, e1 = np.zeros(ls.size, dtype=np.uint64), np.zeros(ls.size, dtype=np.uint64)
        self._check(lib().bwts_members_estimate(self._h, a.ctypes.data, ls.ctypes.data if ls.size else None, None if ws is None else ws.ctypes.data, ls.size,
                                                e0.ctypes.data, e1.ctypes.data))
        return e0.tolist(), e1.tolist()

    def members_estimate_device(self, d_in, lengths, widths=None):
        """bwts_members_estimate_device: the members lie back to back in d_in."""
        ls, ws = _members(lengths, widths)
        e0, e1 = np.zeros(ls.size, dtype=np.uint64), np.zeros(ls.size, dtype=np.uint64)
        self._check(lib().bwts_members_estimate_device(self._h, _ptr(d_in), ls.ctypes.data if ls.size else None, None if ws is None else ws.ctypes.data, ls.size,
                                                       e0.ctypes.data, e1.ctypes.data))
        return e0.tolist(), e1.tolist()

    def pack_members_auto(self, arrays, widths=None, filters=FILTER_AUTO, methods=METHOD_AUTO, out_cap=None):
        """bwts_pack_members_a: pack_members with FILTER_AUTO and METHOD_AUTO allowed, each a scalar for all arrays or a list; the pack
        resolves them by the rules of include/bwts_members.h, and frame_member_filters / frame_member_methods read the choices back."""
        parts = [_bytes_of(a) for a in arrays]
        ls, ws = _members([p.size for p in parts], widths)
        fs, ms = _per_member(ls, filters, "filter"), _per_member(ls, methods, "method")
        a = np.concatenate(parts) if parts else np.empty(0, dtype=np.uint8)
        out = np.empty(pack_members_bound_auto(ls, ws, ms) if out_cap is None else int(out_cap), dtype=np.uint8)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_pack_members_a(self._h, a.ctypes.data, ls.ctypes.data, None if ws is None else ws.ctypes.data, fs.ctypes.data, ms.ctypes.data,
                                              ls.size, out.ctypes.data, out.size, ctypes.byref(got), None, None))
        return out[:got.value].copy()

    def pack_members_auto_device(self, d_in, lengths, widths, d_out, out_cap, filters=FILTER_AUTO, methods=METHOD_AUTO):
        """bwts_pack_members_a_device: (the frame's size in bytes, the resolved filters, the resolved methods)."""
        ls, ws = _members(lengths, widths)
        fs, ms = _per_member(ls, filters, "filter"), _per_member(ls, methods, "method")
        fo, mo = np.zeros(ls.size, dtype=np.uint32), np.zeros(ls.size, dtype=np.uint32)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_pack_members_a_device(self._h, _ptr(d_in), ls.ctypes.data, None if ws is None else ws.ctypes.data, fs.ctypes.data,
                                                     ms.ctypes.data, ls.size, _ptr(d_out), int(out_cap), ctypes.byref(got), fo.ctypes.data, mo.ctypes.data))
        return int(got.value), fo.tolist(), mo.tolist()

    def unpack_members(self, frame, indices=None):
        """bwts_unpack_members: the members named, as a list of bytes, in the order asked (None: all of them); only these are decoded."""
        a = _u8(frame)
        lengths, _ = frame_members(a)
        idx = np.arange(len(lengths), dtype=np.uint64) if indices is None else np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        sizes = [lengths[int(i)] if int(i) < len(lengths) else 0 for i in idx.tolist()]
        total = sum(sizes)
        out = np.empty(max(total, 1), dtype=np.uint8)[:total]       # (never a null pointer: the library judges the indices itself)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_unpack_members(self._h, a.ctypes.data, a.size, idx.ctypes.data if idx.size else None, idx.size, out.ctypes.data, total,
                                              ctypes.byref(got)))
        res, at = [], 0
        for b in sizes:
            res.append(out[at:at + b].tobytes())
            at += b
        return res

    def unpack_members_device(self, d_in, in_bytes, indices, d_out, out_cap):
        """bwts_unpack_members_device: the members named back to back in d_out; returns their sum."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_unpack_members_device(self._h, _ptr(d_in), int(in_bytes), idx.ctypes.data if idx.size else None, idx.size, _ptr(d_out),
                                                     int(out_cap), ctypes.byref(got)))
        return int(got.value)

    # -- members where they lie: tables of device pointers (include/bwts_members.h, "Pointers") ---------
    def gather_device(self, members, lengths, d_out):
        """bwts_gather_device: member k, lengths[k] bytes at members[k] (an int address, a DeviceBuffer, or anything with data_ptr()),
        to d_out, the members back to back."""
        ls, _ = _members(lengths, None)
        ps = _ptrs(members, ls.size)
        self._check(lib().bwts_gather_device(self._h, ps.ctypes.data if ps.size else None, ls.ctypes.data if ls.size else None, ls.size, _ptr(d_out)))

    def scatter_device(self, d_in, members, lengths):
        """bwts_scatter_device: the members that lie back to back in d_in, each to members[k]."""
        ls, _ = _members(lengths, None)
        ps = _ptrs(members, ls.size)
        self._check(lib().bwts_scatter_device(self._h, _ptr(d_in), ps.ctypes.data if ps.size else None, ls.ctypes.data if ls.size else None, ls.size))

    def pack_members_ptrs_device(self, members, lengths, widths, d_out, out_cap, filters=FILTER_AUTO, methods=METHOD_AUTO):
        """bwts_pack_members_p_device: pack_members_auto_device over members where they lie: (the frame's size in bytes, the resolved
        filters, the resolved methods).  The frame is what pack_members_auto_device writes for the same members back to back."""
        ls, ws = _members(lengths, widths)
        ps = _ptrs(members, ls.size)
        fs, ms = _per_member(ls, filters, "filter"), _per_member(ls, methods, "method")
        fo, mo = np.zeros(ls.size, dtype=np.uint32), np.zeros(ls.size, dtype=np.uint32)
        got = ctypes.c_uint64(0)
        self._check(lib().bwts_pack_members_p_device(self._h, ps.ctypes.data if ps.size else None, ls.ctypes.data if ls.size else None,
                                                     None if ws is None else ws.ctypes.data, fs.ctypes.data, ms.ctypes.data, ls.size, _ptr(d_out), int(out_cap),
                                                     ctypes.byref(got), fo.ctypes.data, mo.ctypes.data))
        return int(got.value), fo.tolist(), mo.tolist()

    def unpack_members_ptrs_device(self, d_in, in_bytes, indices, members, dst_bytes):
        """bwts_unpack_members_p_device: member indices[j] of the frame to members[j], of which dst_bytes[j] bytes may be written (only
        the member's own are); indices None: every member in order."""
        room = np.ascontiguousarray(dst_bytes, dtype=np.uint64).reshape(-1)
        ps = _ptrs(members, room.size)
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        if idx is not None and idx.size != room.size:
            raise BwtsError(-1, "one destination per index")
        self._check(lib().bwts_unpack_members_p_device(self._h, _ptr(d_in), int(in_bytes), None if idx is None or not idx.size else idx.ctypes.data, room.size,
                                                       ps.ctypes.data if ps.size else None, room.ctypes.data if room.size else None))

    def pack_tensors(self, tensors, widths=None, filters=FILTER_AUTO, methods=METHOD_AUTO, frame_bytes=1 << 32):
        """A set of device tensors of any sizes as member frames: the set is cut by tensor_frames(sizes, frame_bytes), and every frame
        of the cut is one pack_members_ptrs_device over its pieces where they lie (data_ptr() + offset); returns the frames, one numpy
        uint8 array each, which every reader of member frames takes.  A tensor is anything with data_ptr(), element_size(), numel()
        and is_contiguous(); one that is not contiguous is refused.  widths None takes every tensor's element_size() where that is 1,
        2, 4 or 8, and 1 otherwise: the caller's own dtype, not a guess from the bytes.  filters and methods: a scalar, or one value
        per tensor, carried to all of a tensor's pieces.  One frame buffer on the device, sized for the largest bound, serves all frames."""
        tensors = list(tensors)
        for t in tensors:
            if not t.is_contiguous():
                raise BwtsError(-1, "a tensor that is not contiguous")
        sizes = [int(t.numel()) * int(t.element_size()) for t in tensors]
        ls = np.asarray(sizes, dtype=np.uint64)
        if widths is None:
            widths = [int(t.element_size()) if int(t.element_size()) in (1, 2, 4, 8) else 1 for t in tensors]
        _, ws = _members(ls, widths)
        fs, ms = _per_member(ls, filters, "filter"), _per_member(ls, methods, "method")
        cut = tensor_frames(sizes, frame_bytes)
        sets = [([tensors[k].data_ptr() + off for k, off, _ in fr], [b for _, _, b in fr], [int(ws[k]) for k, _, _ in fr], [int(fs[k]) for k, _, _ in fr],
                 [int(ms[k]) for k, _, _ in fr]) for fr in cut]
        if not sets:
            return []
        cap = max(pack_members_bound_auto(s[1], s[2], s[4]) for s in sets)
        buf = self.alloc(cap)
        try:
            frames = []
            for ptrs, lens, w, f, m in sets:
                got, _, _ = self.pack_members_ptrs_device(ptrs, lens, w, buf, cap, f, m)
                frames.append(buf.download(got))
            return frames
        finally:
            buf.free()

    def unpack_tensors(self, frames, tensors):
        """What pack_tensors made, decoded in place: the frames' own directories (frame_members) are walked against the tensors in
        order, so frame_bytes need not be known.  Every member must lie inside the current tensor's remaining bytes and the members
        must tile the tensors exactly, else BwtsError(-1) before any device call."""
        tensors = list(tensors)
        for t in tensors:
            if not t.is_contiguous():
                raise BwtsError(-1, "a tensor that is not contiguous")
        frames = [_u8(f) for f in frames]
        places = tensor_places([frame_members(f)[0] for f in frames], [int(t.numel()) * int(t.element_size()) for t in tensors])
        if not frames:
            return
        buf = self.alloc(max(f.size for f in frames))
        try:
            for f, pl in zip(frames, places):
                buf.upload(f)
                self.unpack_members_ptrs_device(buf, f.size, None, [tensors[k].data_ptr() + off for k, off, _ in pl], [b for _, _, b in pl])
        finally:
            buf.free()

    def debug_copy_pieces(self, d_src, src_bytes, pieces, d_dst, dst_bytes):
        """bwts_debug_copy_pieces: copy_pieces_kernel alone over (src offset, dst offset, bytes) triples."""
        ps = np.ascontiguousarray(pieces, dtype=np.uint64).reshape(-1, 3)
        self._check(lib().bwts_debug_copy_pieces(self._h, _ptr(d_src), int(src_bytes), ps.ctypes.data if ps.size else None, len(ps), _ptr(d_dst),
                                                 int(dst_bytes)))

    def forward_into(self, a, out):
        """bwts_forward on caller-provided numpy buffers (no allocation inside the call)."""
        self._check(lib().bwts_forward(self._h, a.ctypes.data, a.size, out.ctypes.data))

    def inverse_into(self, a, out):
        self._check(lib().bwts_inverse(self._h, a.ctypes.data, a.size, out.ctypes.data))

    def timings(self):
        t = Timings()
        self._check(lib().bwts_last_timings(self._h, ctypes.byref(t)))
        return t

    # -- harness utilities ---------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def generate(self, kind, seed, n, d_out):
        self._check(lib().bwts_generate_device(self._h, KINDS[kind], int(seed), int(n), _ptr(d_out)))

    def device_equal(self, d_a, d_b, nbytes):
        eq = ctypes.c_int(0)
        self._check(lib().bwts_device_equal(self._h, _ptr(d_a), _ptr(d_b), int(nbytes), ctypes.byref(eq)))
        return bool(eq.value)

    # -- unit-test hooks -------------------------------------------------------------------
    def debug_sort_pairs(self, keys, vals, key_bits=64):
        k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        self._check(lib().bwts_debug_sort_pairs(self._h, k.ctypes.data, v.ctypes.data, k.size, int(key_bits)))
        return k, v

    def debug_rank_steps(self, digits, valid, atomic_items):
        """bwts_debug_rank_steps: (ranks[8][16][64] with 0xffffffff at invalid items, the passes' shipped atomic items)."""
        d = np.ascontiguousarray(digits, dtype=np.uint8).reshape(8, 16, 64)
        v = np.ascontiguousarray(valid, dtype=np.uint8).reshape(8, 16, 64)
        ranks = np.empty((8, 16, 64), dtype=np.uint32)
        shipped = np.zeros(4, dtype=np.uint32)
        self._check(lib().bwts_debug_rank_steps(self._h, d.ctypes.data, v.ctypes.data, int(atomic_items), ranks.ctypes.data, shipped.ctypes.data))
        return ranks, [int(k) for k in shipped]

    def debug_suffix_array(self, data):
        a = _u8(data)
        sa = np.empty(a.size, dtype=np.uint32)
        self._check(lib().bwts_debug_suffix_array(self._h, a.ctypes.data, a.size, sa.ctypes.data))
        return sa

    def debug_lyndon(self, data):
        a = _u8(data)
        st = np.empty(a.size, dtype=np.uint64)
        cnt = ctypes.c_uint64(0)
        self._check(lib().bwts_debug_lyndon(self._h, a.ctypes.data, a.size, st.ctypes.data, st.size, ctypes.byref(cnt)))
        return st[: cnt.value].copy()

    def debug_last_spans(self, cap=4096):
        """Device ms of every timed launch of the most recent call, in launch order (set_timing(2): every launch)."""
        buf = (ctypes.c_double * cap)()
        got = lib().bwts_debug_last_spans(self._h, buf, cap)
        if got < 0:
            self._check(got)
        return [float(buf[i]) for i in range(got)]

    def debug_inverse_report(self):
        """One dict per attempt of the most recent inverse call on this context (INV_REPORT_FIELDS; mark, outcome and form by name,
        the three flags as bool), oldest first."""
        words = len(INV_REPORT_FIELDS)
        buf = (ctypes.c_uint64 * (8 * words))()
        made = ctypes.c_uint64(0)
        got = lib().bwts_debug_inverse_report(self._h, buf, len(buf), ctypes.byref(made))
        if got < 0:
            self._check(got)
        assert got == made.value, "more attempts than records: %d" % made.value
        out = []
        for a in range(got):
            d = {f: int(buf[a * words + i]) for i, f in enumerate(INV_REPORT_FIELDS)}
            d["mark"], d["outcome"], d["form"] = INV_MARKS[d["mark"]], INV_OUTCOMES[d["outcome"]], INV_FORMS[d["form"]]
            for f in ("second_collect", "unit_rank"):
                d[f] = bool(d[f])
            out.append(d)
        return out

    def debug_segments_report(self):
        """What the most recent inverse_segments call on this context did (bwts_debug_segments_report): plan ("lane", "shared", or
        "shared_nomem"), big, runs, segments and bytes by route (lane / shared / single), and the largest attempt count."""
        buf = (ctypes.c_uint64 * 8)()
        self._check(lib().bwts_debug_segments_report(self._h, buf))
        d = _segments_words(buf)
        d["attempts"] = int(buf[7])
        return d

    def debug_forward_report(self):
        """One dict per doubling sort of the most recent forward call on this context (also debug_suffix_array / debug_lyndon), in the
        order they ran: the header (FWD_HEADER_FIELDS; form, keys, no_chunks and end by name, flags as bool; "direct" / "direct_word": header
        word 36 by name and as the number; "lean" / "lean_word": likewise header word 37), "chunks" (FWD_CHUNK_FIELDS), "chunk_S_recut" and "chunk_round_S"
        when the chunk form ran, and "round": one dict per recorded round after round 0 (FWD_ROUND_FIELDS of its form)."""
        buf = (ctypes.c_uint64 * (2 * FWD_SORT_WORDS))()
        made = ctypes.c_uint64(0)
        got = lib().bwts_debug_forward_report(self._h, buf, len(buf), ctypes.byref(made))
        if got < 0:
            self._check(got)
        out = []
        for a in range(got):
            w = [int(v) for v in buf[a * FWD_SORT_WORDS:(a + 1) * FWD_SORT_WORDS]]
            d = {f: w[i] for i, f in enumerate(FWD_HEADER_FIELDS)}
            d["form"], d["keys"], d["no_chunks"], d["end"] = FWD_FORMS[d["form"]], FWD_KEYS[d["keys"]], FWD_NO_CHUNKS[d["no_chunks"]], FWD_ENDS[d["end"]]
            d["direct"], d["direct_word"] = FWD_DIRECT[w[FWD_DIRECT_WORD]], w[FWD_DIRECT_WORD]
            d["lean"], d["lean_word"] = FWD_LEAN[w[FWD_LEAN_WORD]], w[FWD_LEAN_WORD]
            for f in ("cyclic", "varlen", "flags_outside_rank", "rank_early", "need_sa", "order_sort"):
                d[f] = bool(d[f])
            if d["form"] == "chunks":
                d["chunks"] = {f: w[24 + i] for i, f in enumerate(FWD_CHUNK_FIELDS)}
                d["chunk_S_recut"], d["chunk_round_S"] = w[FWD_CHUNK_S_RECUT_WORD], []
                for f in ("wide_possible", "fsl", "enqueued_behind_last"):
                    d["chunks"][f] = bool(d["chunks"][f])
            d["round"] = []
            for r in range(min(max(d["rounds"] - 1, 0), MAX_ROUND_STATS)):
                rw = w[FWD_HEADER_WORDS + r * FWD_ROUND_WORDS:FWD_HEADER_WORDS + (r + 1) * FWD_ROUND_WORDS]
                form = FWD_FORMS[rw[0]]
                rd = {f: rw[i] for i, f in enumerate(FWD_ROUND_FIELDS[form])}
                rd["form"] = form
                if form == "sparse":
                    rd["probe"], rd["whole"], rd["skip_next"] = FWD_PROBES[rd["probe"]], bool(rd["whole"]), bool(rd["skip_next"])
                d["round"].append(rd)
                if d["form"] == "chunks":
                    d["chunk_round_S"].append(rw[FWD_ROUND_CHUNK_S_WORD])
            out.append(d)
        return out


def _segments_words(w):
    """Words 0 .. 6 of bwts_debug_segments_plan / _report as a dict: the plan by name, and segments and bytes by route."""
    plan = SEG_PLANS[int(w[0])]
    own = "shared" if plan == "shared" else "lane"
    d = {"plan": plan, "big": int(w[1]), "runs": int(w[2]), "lane_segments": 0, "lane_bytes": 0, "shared_segments": 0, "shared_bytes": 0,
         "single_segments": int(w[5]), "single_bytes": int(w[6])}
    d[own + "_segments"], d[own + "_bytes"] = int(w[3]), int(w[4])
    return d


def debug_segments_plan(lengths):
    """What inverse_segments would do with segments of these lengths (bwts_debug_segments_plan: host arithmetic, no context, no device):
    the dict of Context.debug_segments_report without "attempts", plus "arena_bytes"."""
    ls = np.ascontiguousarray(lengths, dtype=np.uint64)
    buf = (ctypes.c_uint64 * 8)()
    if lib().bwts_debug_segments_plan(ls.ctypes.data, ls.size, buf) < 0:
        raise BwtsError(-1, "bad segment lengths")
    d = _segments_words(buf)
    d["arena_bytes"] = int(buf[7])
    return d


# bwts_debug_key_plan: the words of the answer ("avg" is a double's bit pattern), and the value of a knob that is not set
KEY_PLAN_FIELDS = ["sigma", "bits", "pad_add", "msym", "key_bits", "varlen", "hstep", "patch_span", "few_ties", "lmax", "kb_iid",
                   "passes_fixed", "passes_var", "avg", "code_built", "kb_var"]
KEY_KNOB_ABSENT = -2 ** 31


def debug_key_plan(hist, n=None, reserve_pad=False, key_symbols=None, varlen=None, key_bits=None, kb_emp=0, partners_of=None):
    """The round-0 key layout a sort picks for a text with this byte histogram (bwts_debug_key_plan: csrc/key_plan.h as host arithmetic,
    no context, no device).  hist: 256 counts, n their sum (the default).  key_symbols, varlen, key_bits: the knobs BWTS_KEY_SYMBOLS,
    BWTS_VARLEN and BWTS_KEY_BITS as numbers or as the text the environment would hold, None for one that is not set.  kb_emp and
    partners_of (65 numbers, negative where the sample has no say): what the key sample found.  Without them the answer is the engine's
    for n < 2^22; from there on the engine may widen the key by its sample.  Returns the dict of KEY_PLAN_FIELDS (flags as bool, "avg"
    as a float) with "codes": the byte -> fixed-width code table, "vlen" and "vcode": length and bits of every byte's code word (all 0
    when no alphabetic code was built)."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.size != 256:
        raise BwtsError(-1, "a histogram has 256 counts")

    def knob(v, is_varlen=False):
        if v is None:
            return KEY_KNOB_ABSENT
        if isinstance(v, str):                     # what atoi makes of the text; BWTS_VARLEN looks at the first character alone
            if is_varlen:
                return {"0": 0, "1": 1}.get(v[:1], 2)
            m = re.match(r"\s*[+-]?\d+", v)
            return int(m.group()) if m else 0
        return int(v)

    pp = None
    if partners_of is not None:
        pp = np.ascontiguousarray(partners_of, dtype=np.float64)
        if pp.size != 65:
            raise BwtsError(-1, "partners_of has 65 entries")
    out = (ctypes.c_uint64 * len(KEY_PLAN_FIELDS))()
    codes, vtab = np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint64)
    rc = lib().bwts_debug_key_plan(h.ctypes.data, int(h.sum()) if n is None else int(n), int(bool(reserve_pad)), knob(key_symbols),
                                   knob(varlen, True), knob(key_bits), int(kb_emp), pp.ctypes.data if pp is not None else None, out,
                                   codes.ctypes.data, vtab.ctypes.data)
    if rc < 0:
        raise BwtsError(-1, "bad histogram or length")
    d = {f: int(out[i]) for i, f in enumerate(KEY_PLAN_FIELDS)}
    d["avg"] = float(np.array([d["avg"]], dtype=np.uint64).view(np.float64)[0])
    for f in ("varlen", "few_ties", "code_built"):
        d[f] = bool(d[f])
    d["codes"], d["vlen"], d["vcode"] = codes, (vtab >> np.uint64(32)).astype(np.int64), (vtab & np.uint64(0xffffffff)).astype(np.int64)
    return d


def debug_mtf_plan(n):
    """How the move-to-front stage cuts one input of n bytes (bwts_debug_mtf_plan: host arithmetic, no context, no device)."""
    buf = (ctypes.c_uint64 * 4)()
    if lib().bwts_debug_mtf_plan(int(n), buf) < 0:
        raise BwtsError(-1, "bad length")
    return {"T": int(buf[0]), "G": int(buf[1]), "tiles": int(buf[2]), "groups": int(buf[3])}


def debug_ec_plan(n):
    """How the entropy coder cuts one input of n bytes (bwts_debug_ec_plan: host arithmetic, no context, no device)."""
    buf = (ctypes.c_uint64 * 5)()
    if lib().bwts_debug_ec_plan(int(n), buf) < 0:
        raise BwtsError(-1, "bad length")
    return {"T": int(buf[0]), "K": int(buf[1]), "tiles": int(buf[2]), "blocks": int(buf[3]), "bound": int(buf[4])}


def debug_crc_plan(n):
    """How the checksum cuts one input of n bytes (bwts_debug_crc_plan: host arithmetic, no context, no device)."""
    buf = (ctypes.c_uint64 * 4)()
    if lib().bwts_debug_crc_plan(int(n), buf) < 0:
        raise BwtsError(-1, "bad length")
    return {"T": int(buf[0]), "G": int(buf[1]), "tiles": int(buf[2]), "groups": int(buf[3])}


def debug_zrl_plan(n):
    """How the zero-run stage cuts one input of n bytes (bwts_debug_zrl_plan: host arithmetic, no context, no device)."""
    buf = (ctypes.c_uint64 * 2)()
    if lib().bwts_debug_zrl_plan(int(n), buf) < 0:
        raise BwtsError(-1, "bad length")
    return {"T": int(buf[0]), "tiles": int(buf[1])}


def debug_planes_plan(n, width):
    """How the byte-plane split cuts one input of n bytes at a width (bwts_debug_planes_plan: host arithmetic, no context, no device)."""
    buf = (ctypes.c_uint64 * 4)()
    if lib().bwts_debug_planes_plan(int(n), int(width), buf) < 0:
        raise BwtsError(-1, "bad length or width")
    return {"T": int(buf[0]), "tiles": int(buf[1]), "q": int(buf[2]), "tail": int(buf[3])}


def zrl_bound(n):
    """bwts_zrl_bound: the most bytes the zero-run stage writes for an input of n bytes: n."""
    b = int(lib().bwts_zrl_bound(int(n)))
    if b == 0:
        raise BwtsError(-5 if int(n) > 0 else -1, "no bound for this length")
    return b


def _pack_version(version, planes):
    """The frame version a pack is asked for: 1 unless named; planes alone means 3, and goes with no other version."""
    if planes is None:
        return 1 if version is None else int(version)
    if version is not None and int(version) != 3:
        raise BwtsError(-1, "planes asks for a frame of version 3")
    return 3


def pack_bound(n, block_bytes=0, version=None, planes=None):
    """bwts_pack_bound_v: the largest frame of the given version an input of n bytes cut at block_bytes can have; with planes=2, 4 or 8
    bwts_pack_planes_bound (version 3)."""
    version = _pack_version(version, planes)
    if planes is None:
        b = int(lib().bwts_pack_bound_v(version, int(n), int(block_bytes)))
    else:
        b = int(lib().bwts_pack_planes_bound(int(planes), int(n), int(block_bytes)))
    if b == 0:
        raise BwtsError(-5 if int(n) > (1 << 32) else -1, "no bound for these arguments")
    return b


def _bytes_of(a):
    """A member as its bytes: a numpy array of any dtype is viewed, not converted."""
    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return np.frombuffer(bytes(a), dtype=np.uint8)


def _members(lengths, widths):
    """Lengths and widths of a member call as the arrays the library takes; widths None stays None (all 1)."""
    ls = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
    if widths is None:
        return ls, None
    ws = np.ascontiguousarray(widths, dtype=np.uint32).reshape(-1)
    if ws.size != ls.size:
        raise BwtsError(-1, "one width per member")
    return ls, ws


def _filters(ls, filters):
    """The filters of a member call as the array the library takes; None stays None (no filter)."""
    if filters is None:
        return None
    fs = np.ascontiguousarray(filters, dtype=np.uint32).reshape(-1)
    if fs.size != ls.size:
        raise BwtsError(-1, "one filter per member")
    return fs


def _members_f(lengths, widths, filters):
    """Lengths, widths and filters of a segment call of the delta filter: all three named."""
    if widths is None or filters is None:
        raise BwtsError(-1, "a width and a filter per segment")
    ls, ws = _members(lengths, widths)
    return ls, ws, _filters(ls, filters)


def _methods(ls, methods):
    """The methods of a member call as the array the library takes; None stays None (the whole chain)."""
    if methods is None:
        return None
    ms = np.ascontiguousarray(methods, dtype=np.uint32).reshape(-1)
    if ms.size != ls.size:
        raise BwtsError(-1, "one method per member")
    return ms


def pack_members_bound(lengths, widths=None, methods=None):
    """bwts_pack_members_bound_m: the largest member frame of members of these lengths (and, where methods are named, widths)."""
    ls, ws = _members(lengths, widths)
    ms = _methods(ls, methods)
    if ms is None:
        b = int(lib().bwts_pack_members_bound(ls.ctypes.data if ls.size else None, ls.size))
    else:
        b = int(lib().bwts_pack_members_bound_m(ls.ctypes.data if ls.size else None, None if ws is None else ws.ctypes.data, ms.ctypes.data, ls.size))
    if b == 0:
        bad = ls.size == 0 or bool((ls == 0).any()) or (ms is not None and (bool((ms > 1).any()) or (ws is not None and not bool(np.isin(ws, (1, 2, 4, 8)).all()))))
        raise BwtsError(-1 if bad else -5, "no bound for these lengths")
    return b


def _per_member(ls, value, what):
    """A filter or a method of an auto pack as the array the library takes: a scalar for all members, or one per member."""
    if np.ndim(value) == 0:
        return np.full(ls.size, int(value), dtype=np.uint32)
    vs = np.ascontiguousarray(value, dtype=np.uint32).reshape(-1)
    if vs.size != ls.size:
        raise BwtsError(-1, "one %s per member" % what)
    return vs


def pack_members_bound_auto(lengths, widths=None, methods=METHOD_AUTO):
    """bwts_pack_members_bound_a: the largest frame an auto pack of these members can make: a METHOD_AUTO member counts with the larger
    of its two bounds."""
    ls, ws = _members(lengths, widths)
    ms = _per_member(ls, methods, "method")
    b = int(lib().bwts_pack_members_bound_a(ls.ctypes.data if ls.size else None, None if ws is None else ws.ctypes.data, ms.ctypes.data, ls.size))
    if b == 0:
        bad = ls.size == 0 or bool((ls == 0).any()) or bool(((ms > 1) & (ms != METHOD_AUTO)).any()) or (ws is not None and not bool(np.isin(ws, (1, 2, 4, 8)).all()))
        raise BwtsError(-1 if bad else -5, "no bound for these lengths")
    return b


def frame_members(frame):
    """bwts_frame_members: (lengths, widths) of a member frame, two lists, from its header and directory (host arithmetic)."""
    a = _u8(frame)
    count = ctypes.c_uint64(0)
    rc = lib().bwts_frame_members(a.ctypes.data, a.size, None, None, 0, ctypes.byref(count))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    ls, ws = np.zeros(count.value, dtype=np.uint64), np.zeros(count.value, dtype=np.uint32)
    rc = lib().bwts_frame_members(a.ctypes.data, a.size, ls.ctypes.data, ws.ctypes.data, ls.size, ctypes.byref(count))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    return ls.tolist(), ws.tolist()


def frame_member_filters(frame):
    """bwts_frame_members_f: the members' filters, a list (all 0 for a version-1 frame), from header and directory (host arithmetic)."""
    a = _u8(frame)
    count = ctypes.c_uint64(0)
    rc = lib().bwts_frame_members_f(a.ctypes.data, a.size, None, None, None, 0, ctypes.byref(count))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    fs = np.zeros(count.value, dtype=np.uint32)
    rc = lib().bwts_frame_members_f(a.ctypes.data, a.size, None, None, fs.ctypes.data, fs.size, ctypes.byref(count))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    return fs.tolist()


def frame_member_methods(frame):
    """bwts_frame_members_m: the members' methods, a list (all 0 below version 3), from header and directory (host arithmetic)."""
    a = _u8(frame)
    count = ctypes.c_uint64(0)
    rc = lib().bwts_frame_members_m(a.ctypes.data, a.size, None, None, None, None, 0, ctypes.byref(count))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    ms = np.zeros(count.value, dtype=np.uint32)
    rc = lib().bwts_frame_members_m(a.ctypes.data, a.size, None, None, None, ms.ctypes.data, ms.size, ctypes.byref(count))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    return ms.tolist()


MAX_MEMBERS = 1 << 20           # the most members of one frame (include/bwts_members.h)


def _ptrs(members, count):
    """Members where they lie, as the uint64 array that is a table of device pointers: int addresses, DeviceBuffers, or anything with data_ptr()."""
    ps = np.asarray([_ptr(m) for m in members], dtype=np.uint64).reshape(-1)
    if ps.size != count:
        raise BwtsError(-1, "one pointer per member")
    return ps


def tensor_frames(lengths, frame_bytes=1 << 32):
    """The cut of a set of tensors of these byte lengths into member frames, as pure arithmetic: a list of frames, each a list of
    (tensor index, byte offset, bytes) in order.  A zero-length tensor is in no frame.  A tensor of at most frame_bytes bytes joins the
    current frame if the frame's sum stays <= frame_bytes and its member count <= 2^20, else it opens a new one.  A longer tensor
    closes the current frame and is cut into pieces of frame_bytes rounded down to a multiple of 8, each a frame of its own; the
    last, shorter piece opens a frame that later tensors may join."""
    fb = int(frame_bytes)
    if fb < 8 or fb > 1 << 32:
        raise BwtsError(-1, "frame_bytes outside [8, 2^32]")
    piece = fb // 8 * 8
    frames, cur, total = [], [], 0
    for k, n in enumerate(lengths):
        n = int(n)
        if n < 0:
            raise BwtsError(-1, "a negative length")
        if n == 0:
            continue
        if n > fb:
            if cur:
                frames.append(cur)
            cur, total, at = [], 0, 0
            while n - at > piece:
                frames.append([(k, at, piece)])
                at += piece
            cur, total = [(k, at, n - at)], n - at
            continue
        if cur and (total + n > fb or len(cur) >= MAX_MEMBERS):
            frames.append(cur)
            cur, total = [], 0
        cur.append((k, 0, n))
        total += n
    if cur:
        frames.append(cur)
    return frames


def tensor_places(frame_lengths, tensor_bytes):
    """The members of frames (frame_lengths: a list of member lengths per frame) laid over tensors of tensor_bytes bytes in order: per
    frame a list of (tensor index, byte offset, bytes).  BwtsError(-1) unless every member lies inside the current tensor's remaining
    bytes and the members tile the tensors exactly (zero-length tensors are passed over)."""
    k, at, out = 0, 0, []
    sizes = [int(b) for b in tensor_bytes]
    for lens in frame_lengths:
        places = []
        for n in lens:
            n = int(n)
            while k < len(sizes) and at == sizes[k]:
                k, at = k + 1, 0
            if k == len(sizes):
                raise BwtsError(-1, "more members than the tensors hold")
            if n > sizes[k] - at:
                raise BwtsError(-1, "a member of %d bytes straddles the end of tensor %d" % (n, k))
            places.append((k, at, n))
            at += n
        out.append(places)
    while k < len(sizes) and at == sizes[k]:
        k, at = k + 1, 0
    if k != len(sizes):
        raise BwtsError(-1, "the members end inside tensor %d" % k)
    return out


def _ranges(ranges):
    """(offset, nbytes) pairs as the uint64 array that is a bwts_range list."""
    return np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)


def debug_unpack_ranges_plan(frame, ranges, out_cap=None, in_bytes=None):
    """What a range read of this frame would decode and move (bwts_debug_unpack_ranges_plan: host arithmetic over the frame's header
    and directory, no context, no device): blocks, runs [(first block, blocks)], covered_bytes, stream_bytes, coded_bytes, out_bytes,
    T, streams and out [(src, dst, bytes)].  Refusals raise BwtsError with the call's code.  in_bytes: the frame's length where `frame`
    holds its header and directory alone."""
    a, rs = _u8(frame), _ranges(ranges)
    nbytes = a.size if in_bytes is None else int(in_bytes)
    cap = (1 << 64) - 1 if out_cap is None else int(out_cap)
    head = (ctypes.c_uint64 * 8)()
    rp = rs.ctypes.data if rs.size else None
    rc = lib().bwts_debug_unpack_ranges_plan(a.ctypes.data, nbytes, rp, len(rs), cap, head, None, 0)
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    lists = np.zeros(int(head[7]), dtype=np.uint64)
    rc = lib().bwts_debug_unpack_ranges_plan(a.ctypes.data, nbytes, rp, len(rs), cap, head, lists.ctypes.data, lists.size)
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    runs, w = int(head[1]), lists.tolist()
    triples = [tuple(w[2 * runs + 3 * i:2 * runs + 3 * i + 3]) for i in range(runs + len(rs))]
    return {"blocks": int(head[0]), "runs": [tuple(w[2 * i:2 * i + 2]) for i in range(runs)], "covered_bytes": int(head[2]),
            "stream_bytes": int(head[3]), "coded_bytes": int(head[4]), "out_bytes": int(head[5]), "T": int(head[6]),
            "streams": triples[:runs], "out": triples[runs:]}


def unpack_size(frame):
    """bwts_unpack_size: (n, frame_bytes) of the frame at the start of a byte string, from its header and directory."""
    a = _u8(frame)
    n, fb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().bwts_unpack_size(a.ctypes.data, a.size, ctypes.byref(n), ctypes.byref(fb))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    return int(n.value), int(fb.value)


def ec_bound(n):
    """bwts_ec_bound: the largest stream an input of n bytes can have."""
    b = int(lib().bwts_ec_bound(int(n)))
    if b == 0:
        raise BwtsError(-5 if int(n) > 0 else -1, "no bound for this length")
    return b


def ec_bound_segments(lengths):
    ls = np.ascontiguousarray(lengths, dtype=np.uint64)
    got = ctypes.c_uint64(0)
    rc = lib().bwts_ec_bound_segments(ls.ctypes.data, ls.size, ctypes.byref(got))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    return int(got.value)


def ec_decoded_size(stream):
    """bwts_ec_decoded_size: the n a stream's header names, checked against the stream's length."""
    a = _u8(stream)
    head = np.zeros(16, dtype=np.uint8)
    head[:min(a.size, 16)] = a[:16]
    got = ctypes.c_uint64(0)
    rc = lib().bwts_ec_decoded_size(head.ctypes.data, a.size, ctypes.byref(got))
    if rc != 0:
        raise BwtsError(rc, lib().bwts_strerror(rc).decode())
    return int(got.value)


def _ptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):      # torch tensor on the context's GPU
        return x.data_ptr()
    return int(x)


def mk_bwts(data, device=0):
    """Forward bijective BWT of ``data`` (bytes-like) -> numpy uint8 array of the same length."""
    with Context(device) as ctx:
        return ctx.forward(data)


def unbwts(data, device=0):
    """Inverse bijective BWT of ``data`` (bytes-like) -> numpy uint8 array of the same length."""
    with Context(device) as ctx:
        return ctx.inverse(data)
