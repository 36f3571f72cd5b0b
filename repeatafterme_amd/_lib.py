"""ctypes loader for libramx.so (include/ramx.h, include/ramx_dist.h, include/ramx_xfam.h).  Fails loudly: there is no CPU path."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAMX_LIB") or os.path.join(_PKG, "libramx.so")   # RAMX_LIB: A/B builds (tools/build_variant.sh)
CLI_PATH = os.path.join(_PKG, "RAMExtend")

# every symbol include/ramx.h declares (tests/test_cabi.py checks the .so exports all of them)
EXPORTS = [
    "ramx_set_runtime", "ramx_extend_alignment", "ramx_extend_flat", "ramx_invalidate_library", "ramx_preload_library", "ramx_resolve_flanks", "ramx_last_error", "ramx_device_count",
    "ramx_dev_create", "ramx_dev_destroy", "ramx_dev_load_library", "ramx_dev_begin_direction",
    "ramx_dev_run_direction", "ramx_dev_download", "ramx_dev_peek_state", "ramx_dev_peek_windows", "ramx_dev_peek_family_state", "ramx_dev_set_row_trace", "ramx_dev_run_families", "ramx_extend_batch", "ramx_comm_unique_id",
    "ramx_dev_comm_init", "ramx_dev_comm_size", "ramx_dev_set_allreduce_cb", "ramx_dev_peer_export", "ramx_dev_peer_import",
    "ramx_dev_peer_selftest", "ramx_dev_peer_enable", "ramx_dev_hostbox_attach", "ramx_hostbox_unlink", "ramx_get_matrix", "ramx_get_matrix_using_gap_penalties",
    "ramx_get_repeatscout_matrix", "ramx_free_scoring_system", "ramx_calculate_lambda",
    "ramx_load_sequence_subset_minimal", "ramx_load_sequence_subset_packed", "ramx_packed_decode", "ramx_dev_load_library_packed", "ramx_preload_library_packed", "ramx_free_library", "ramx_overlap_avoidance",
    "ramx_print_core_edges", "ramx_allocate_score", "ramx_free_score", "ramx_cli_main",
    "ramx_dev_profile", "ramx_set_profile_sink",
    "ramx_dev_align", "ramx_set_align_sink",
    "ramx_dev_pileup", "ramx_recall_consensus", "ramx_dev_refine", "ramx_set_refine_sink",
    "ramx_dev_dinuc", "ramx_recall_cpg", "ramx_dev_refine_cpg", "ramx_set_cpg_sink",
    "ramx_dev_copy_stats", "ramx_copy_kimura", "ramx_family_divergence", "ramx_set_copies_sink",
    "ramx_dev_planes", "ramx_dev_plane_gram", "ramx_dev_plane_gram_ms", "ramx_select_planes", "ramx_link_pairs", "ramx_set_linkage_sink",
    "ramx_link_components", "ramx_dev_subfamilies", "ramx_dev_subfam_masks", "ramx_dev_subfam_ms", "ramx_set_subfam_sink",
    "ramx_dev_tsd", "ramx_tsd_sites", "ramx_tsd_summary", "ramx_termini", "ramx_tsd_flat", "ramx_tsd_alignment", "ramx_tsd_batch",
    "ramx_dev_period", "ramx_period_sequence", "ramx_period_segments", "ramx_period_summary", "ramx_period_flat", "ramx_period_alignment", "ramx_period_batch",
    "ramx_dev_term", "ramx_term_pair", "ramx_term_summary", "ramx_term_flat", "ramx_term_alignment", "ramx_term_batch",
]

# every symbol include/ramx_dist.h declares (tests/test_cabi_dist.py checks the .so exports all of them)
EXPORTS_DIST = [
    "ramx_dev_copy_dist", "ramx_dev_copy_dist_ms", "ramx_select_copies", "ramx_dist_kimura", "ramx_dist_summary", "ramx_set_dist_sink",
]

# every symbol include/ramx_xfam.h declares (tests/test_cabi_xfam.py checks the .so exports all of them)
EXPORTS_XFAM = [
    "ramx_seq_pair_host", "ramx_dev_seq_pairs", "ramx_xfam_candidates", "ramx_xfam_groups",
]


class RamxError(RuntimeError):
    pass


class FlatCores(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in
                ("left_pos", "right_pos", "lower", "upper", "orient", "left_ext", "right_ext",
                 "left_len", "right_len", "score")]


class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("bandwidth", "cappenalty", "minimprovement", "L", "when_to_stop",
                                          "l", "gapopen", "gapextn")] + [("matrix", C.c_void_p)]


class RunInfo(C.Structure):
    _fields_ = [("ret", C.c_int32), ("rows_executed", C.c_int32), ("limit_warning", C.c_int32),
                ("overflow32", C.c_int32), ("n_extendable", C.c_int32), ("launches", C.c_int32),
                ("loop_ms", C.c_double), ("kernel_ms_avg", C.c_double), ("kernel_samples", C.c_int32),
                ("prep_ms", C.c_double), ("persistent", C.c_int32), ("lanes_per_flank", C.c_int32),
                ("respeculated_rows", C.c_int32), ("packed_rows", C.c_int32), ("lean_rows", C.c_int32)]


class Family(C.Structure):
    _fields_ = [("cores", FlatCores), ("sequence", C.c_void_p), ("seq_len", C.c_uint64), ("master", C.c_void_p)]


class Flank(C.Structure):
    _fields_ = [("start", C.c_int64), ("t_lo", C.c_int32), ("t_hi", C.c_int32), ("step", C.c_int8),
                ("compl_", C.c_int8), ("pad_", C.c_int8 * 6)]


ALLREDUCE_CB = C.CFUNCTYPE(None, C.POINTER(C.c_longlong), C.c_void_p)


class ProfileRec(C.Structure):      # ramx_profile
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "n_cols", "ret", "n_flanks")] + \
               [("cols", C.c_void_p), ("core_index", C.c_void_p), ("last_uncapped_row", C.c_void_p)]


PROFILE_CB = C.CFUNCTYPE(None, C.POINTER(ProfileRec), C.c_void_p)


class AlignRec(C.Structure):        # ramx_alignment
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "n_flanks", "stride")] + \
               [(k, C.c_void_p) for k in ("cons", "flanks", "core_index", "ends", "col_idx", "col_ins")]


ALIGN_CB = C.CFUNCTYPE(None, C.POINTER(AlignRec), C.c_void_p)


class RefineRec(C.Structure):       # ramx_refinement
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "refined_rows", "replays", "converged", "n_flanks", "pad_")] + \
               [(k, C.c_void_p) for k in ("cons", "cols", "refined_cons", "refined_cols")]


REFINE_CB = C.CFUNCTYPE(None, C.POINTER(RefineRec), C.c_void_p)


class CpgRec(C.Structure):          # ramx_cpg_refinement
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "refined_rows", "replays", "converged", "n_flanks", "n_cpg")] + \
               [(k, C.c_void_p) for k in ("cons", "refined_cons", "refined_cols", "refined_di")]


CPG_CB = C.CFUNCTYPE(None, C.POINTER(CpgRec), C.c_void_p)


class CopyStats(C.Structure):       # ramx_copy_stats
    _fields_ = [(k, C.c_int32) for k in ("cols", "match", "ts", "tv", "n_match", "del_", "del_open", "ins", "ins_open", "cpg_cols",
                                          "cpg_ts", "score")]


class CopiesRec(C.Structure):       # ramx_copies
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "n_flanks")] + \
               [(k, C.c_void_p) for k in ("cons", "flanks", "core_index", "ends", "stats")]


COPIES_CB = C.CFUNCTYPE(None, C.POINTER(CopiesRec), C.c_void_p)


class Plane(C.Structure):           # ramx_plane
    _fields_ = [("row", C.c_int32), ("cls", C.c_int32)]


class Link(C.Structure):            # ramx_link
    _fields_ = [(k, C.c_int32) for k in ("p", "q", "n", "n_p", "n_q", "n_pq")] + [("expected", C.c_double), ("mlog10p", C.c_double)]


class LinkageRec(C.Structure):      # ramx_linkage
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "n_planes")] + \
               [(k, C.c_void_p) for k in ("cons", "cols", "planes", "co")]


LINKAGE_CB = C.CFUNCTYPE(None, C.POINTER(LinkageRec), C.c_void_p)


class SubfamGroup(C.Structure):     # ramx_subfam_group
    _fields_ = [(k, C.c_int32) for k in ("group", "size", "refined_rows", "replays", "converged")] + \
               [(k, C.c_void_p) for k in ("refined_cons", "refined_cols")]


class SubfamRec(C.Structure):       # ramx_subfamilies
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "n_flanks", "n_planes", "n_variants", "K", "iterations",
                                         "converged", "n_groups")] + \
               [(k, C.c_void_p) for k in ("cons", "flanks", "core_index", "planes", "labels", "patterns", "cnt", "size", "dist")] + \
               [("groups", C.POINTER(SubfamGroup))]


SUBFAM_CB = C.CFUNCTYPE(None, C.POINTER(SubfamRec), C.c_void_p)


class TsdParams(C.Structure):       # ramx_tsd_params
    _fields_ = [(k, C.c_int32) for k in ("slack", "kmin", "kmax", "mm_div")]


class TsdHist(C.Structure):         # ramx_tsd_hist
    _fields_ = [("hist", C.c_int32 * 33), ("mode", C.c_int32), ("mode_count", C.c_int32), ("pad_", C.c_int32), ("null", C.c_double * 33)]


class PeriodParams(C.Structure):    # ramx_period_params
    _fields_ = [(k, C.c_int32) for k in ("pmax", "mm", "min_score", "reserved")]


class PeriodHist(C.Structure):      # ramx_period_hist
    _fields_ = [(k, C.c_int32) for k in ("n", "n_tract", "n_mono", "n_simple", "n_tandem", "at_lo", "at_hi", "mode", "mode_count")] + \
               [("reserved", C.c_int32 * 3)]


class TermParams(C.Structure):      # ramx_term_params
    _fields_ = [(k, C.c_int32) for k in ("tmax", "match", "mismatch", "gap", "min_score", "slack")] + [("reserved", C.c_int32 * 2)]


class TermFamily(C.Structure):      # ramx_term_family
    _fields_ = [(k, C.c_int32) for k in ("n", "n_direct", "n_inverted", "direct_anchored", "inverted_anchored", "direct_median",
                                         "inverted_median", "verdict")] + \
               [(k, C.c_int64) for k in ("direct_matches", "direct_columns", "inverted_matches", "inverted_columns")]


class CopyDistRec(C.Structure):     # ramx_copy_dist
    _fields_ = [(k, C.c_int32) for k in ("cover", "sites", "ts", "tv", "del_one", "del_both")]


class DistFamily(C.Structure):      # ramx_dist_family
    _fields_ = [(k, C.c_int32) for k in ("n", "pairs", "used", "medoid")] + [("mean", C.c_double), ("medoid_mean", C.c_double)]


class DistRec(C.Structure):         # ramx_dist
    _fields_ = [(k, C.c_int32) for k in ("direction", "family", "rows", "n_flanks", "n_copies")] + \
               [(k, C.c_void_p) for k in ("cons", "core_index", "ends", "copies", "dist")]


DIST_CB = C.CFUNCTYPE(None, C.POINTER(DistRec), C.c_void_p)


class PairParams(C.Structure):      # ramx_pair_params
    _fields_ = [(k, C.c_int32) for k in ("match", "mismatch", "gap", "min_score")]


class SeqPair(C.Structure):         # ramx_seq_pair
    _fields_ = [(k, C.c_int32) for k in ("a", "b", "inverted", "reserved")]


class XfamLinkParams(C.Structure):  # ramx_xfam_link_params
    _fields_ = [(k, C.c_int32) for k in ("min_columns", "min_permille")]


def build(force: bool = False) -> None:
    """Compile libramx.so + RAMExtend in-tree (hipcc --offload-arch=gfx950, gcc)."""
    if force or not os.path.exists(LIB_PATH) or not os.path.exists(CLI_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(_PKG, "csrc"), "all"])


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RamxError(f"{LIB_PATH} is missing: build it with `make -C repeatafterme_amd/csrc` "
                            "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.ramx_last_error.restype = C.c_char_p
        L.ramx_set_runtime.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ramx_set_runtime.restype = None
        L.ramx_extend_flat.argtypes = [C.c_int, C.POINTER(FlatCores), C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.POINTER(Params), C.POINTER(RunInfo)]
        L.ramx_extend_flat.restype = C.c_int
        L.ramx_resolve_flanks.argtypes = [C.c_int, C.POINTER(FlatCores), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.ramx_resolve_flanks.restype = C.c_int
        L.ramx_extend_batch.argtypes = [C.c_int, C.POINTER(Family), C.c_int32, C.POINTER(Params), C.POINTER(RunInfo)]
        L.ramx_extend_batch.restype = C.c_int
        L.ramx_device_count.restype = C.c_int
        L.ramx_dev_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.ramx_dev_destroy.argtypes = [C.c_void_p]
        L.ramx_dev_destroy.restype = None
        L.ramx_dev_load_library.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.ramx_dev_begin_direction.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params)]
        L.ramx_dev_run_direction.argtypes = [C.c_void_p, C.POINTER(RunInfo)]
        L.ramx_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.ramx_dev_peek_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)]
        L.ramx_dev_peek_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32)]
        L.ramx_dev_peek_family_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.ramx_comm_unique_id.argtypes = [C.c_void_p]
        L.ramx_dev_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ramx_dev_comm_size.argtypes = [C.c_void_p]
        L.ramx_dev_set_allreduce_cb.argtypes = [C.c_void_p, ALLREDUCE_CB, C.c_void_p]
        L.ramx_dev_peer_export.argtypes = [C.c_void_p, C.c_void_p]
        L.ramx_dev_peer_import.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.ramx_dev_peer_selftest.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
        L.ramx_dev_peer_enable.argtypes = [C.c_void_p, C.c_int]
        L.ramx_dev_hostbox_attach.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
        L.ramx_hostbox_unlink.argtypes = [C.c_char_p]
        L.ramx_dev_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_double)]
        L.ramx_dev_profile.restype = C.c_int
        L.ramx_set_profile_sink.argtypes = [PROFILE_CB, C.c_void_p]
        L.ramx_set_profile_sink.restype = None
        L.ramx_dev_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_align.restype = C.c_int
        L.ramx_set_align_sink.argtypes = [ALIGN_CB, C.c_void_p]
        L.ramx_set_align_sink.restype = None
        L.ramx_dev_pileup.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_pileup.restype = C.c_int
        L.ramx_recall_consensus.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.ramx_recall_consensus.restype = C.c_int32
        L.ramx_dev_refine.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                      C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_refine.restype = C.c_int
        L.ramx_set_refine_sink.argtypes = [REFINE_CB, C.c_void_p, C.c_int32]
        L.ramx_set_refine_sink.restype = None
        L.ramx_dev_dinuc.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_dinuc.restype = C.c_int
        L.ramx_recall_cpg.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.POINTER(C.c_int32)]
        L.ramx_recall_cpg.restype = C.c_int32
        L.ramx_dev_refine_cpg.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_refine_cpg.restype = C.c_int
        L.ramx_set_cpg_sink.argtypes = [CPG_CB, C.c_void_p, C.c_int32, C.c_int32]
        L.ramx_set_cpg_sink.restype = None
        L.ramx_dev_copy_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_copy_stats.restype = C.c_int
        L.ramx_copy_kimura.argtypes = [C.c_void_p]
        L.ramx_copy_kimura.restype = C.c_double
        L.ramx_family_divergence.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
        L.ramx_family_divergence.restype = C.c_double
        L.ramx_set_copies_sink.argtypes = [COPIES_CB, C.c_void_p]
        L.ramx_set_copies_sink.restype = None
        L.ramx_dev_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Params),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_planes.restype = C.c_int
        L.ramx_dev_plane_gram.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.ramx_dev_plane_gram.restype = C.c_int
        L.ramx_dev_plane_gram_ms.argtypes = [C.c_void_p]
        L.ramx_dev_plane_gram_ms.restype = C.c_double
        L.ramx_select_planes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.ramx_select_planes.restype = C.c_int32
        L.ramx_link_pairs.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_int32]
        L.ramx_link_pairs.restype = C.c_int32
        L.ramx_set_linkage_sink.argtypes = [LINKAGE_CB, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.ramx_set_linkage_sink.restype = None
        L.ramx_set_subfam_sink.argtypes = [SUBFAM_CB, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32]
        L.ramx_set_subfam_sink.restype = None
        L.ramx_link_components.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.ramx_link_components.restype = C.c_int32
        L.ramx_dev_subfamilies.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_subfamilies.restype = C.c_int
        L.ramx_dev_subfam_masks.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.ramx_dev_subfam_masks.restype = C.c_int
        L.ramx_dev_subfam_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.ramx_dev_subfam_ms.restype = None
        L.ramx_dev_tsd.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TsdParams), C.c_void_p, C.POINTER(C.c_double)]
        L.ramx_dev_tsd.restype = C.c_int
        L.ramx_tsd_sites.argtypes = [C.POINTER(FlatCores), C.c_void_p]
        L.ramx_tsd_sites.restype = C.c_int32
        L.ramx_tsd_summary.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TsdParams), C.POINTER(TsdHist)]
        L.ramx_tsd_summary.restype = C.c_int
        L.ramx_termini.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, C.POINTER(C.c_int32)]
        L.ramx_termini.restype = C.c_int
        L.ramx_tsd_flat.argtypes = [C.POINTER(FlatCores), C.c_void_p, C.c_uint64, C.POINTER(TsdParams), C.c_void_p]
        L.ramx_tsd_flat.restype = C.c_int
        L.ramx_tsd_alignment.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TsdParams), C.c_void_p]
        L.ramx_tsd_alignment.restype = C.c_int
        L.ramx_tsd_batch.argtypes = [C.POINTER(Family), C.c_int32, C.POINTER(TsdParams), C.c_void_p]
        L.ramx_tsd_batch.restype = C.c_int
        L.ramx_dev_period.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(PeriodParams), C.c_void_p, C.POINTER(C.c_double)]
        L.ramx_dev_period.restype = C.c_int
        L.ramx_period_sequence.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PeriodParams), C.c_void_p]
        L.ramx_period_sequence.restype = C.c_int
        L.ramx_period_segments.argtypes = [C.POINTER(FlatCores), C.c_int32, C.c_void_p]
        L.ramx_period_segments.restype = C.c_int32
        L.ramx_period_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(PeriodParams), C.POINTER(PeriodHist)]
        L.ramx_period_summary.restype = C.c_int
        L.ramx_period_flat.argtypes = [C.POINTER(FlatCores), C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(PeriodParams), C.c_void_p]
        L.ramx_period_flat.restype = C.c_int
        L.ramx_period_alignment.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(PeriodParams), C.c_void_p]
        L.ramx_period_alignment.restype = C.c_int
        L.ramx_period_batch.argtypes = [C.POINTER(Family), C.c_int32, C.c_int32, C.POINTER(PeriodParams), C.c_void_p]
        L.ramx_period_batch.restype = C.c_int
        L.ramx_dev_term.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(TermParams), C.c_void_p, C.POINTER(C.c_double)]
        L.ramx_dev_term.restype = C.c_int
        L.ramx_term_pair.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(TermParams), C.c_void_p]
        L.ramx_term_pair.restype = C.c_int
        L.ramx_term_summary.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TermParams), C.POINTER(TermFamily)]
        L.ramx_term_summary.restype = C.c_int
        L.ramx_term_flat.argtypes = [C.POINTER(FlatCores), C.c_void_p, C.c_uint64, C.POINTER(TermParams), C.c_void_p]
        L.ramx_term_flat.restype = C.c_int
        L.ramx_term_alignment.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TermParams), C.c_void_p]
        L.ramx_term_alignment.restype = C.c_int
        L.ramx_term_batch.argtypes = [C.POINTER(Family), C.c_int32, C.POINTER(TermParams), C.c_void_p]
        L.ramx_term_batch.restype = C.c_int
        L.ramx_dev_copy_dist.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ramx_dev_copy_dist.restype = C.c_int
        L.ramx_dev_copy_dist_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.ramx_dev_copy_dist_ms.restype = None
        L.ramx_select_copies.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        L.ramx_select_copies.restype = C.c_int32
        L.ramx_dist_kimura.argtypes = [C.c_void_p]
        L.ramx_dist_kimura.restype = C.c_double
        L.ramx_dist_summary.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(DistFamily)]
        L.ramx_dist_summary.restype = C.c_int
        L.ramx_set_dist_sink.argtypes = [DIST_CB, C.c_void_p, C.c_int32, C.c_int32]
        L.ramx_set_dist_sink.restype = None
        L.ramx_seq_pair_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(PairParams), C.c_void_p]
        L.ramx_seq_pair_host.restype = C.c_int
        L.ramx_dev_seq_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(PairParams),
                                         C.c_void_p, C.POINTER(C.c_double)]
        L.ramx_dev_seq_pairs.restype = C.c_int
        L.ramx_xfam_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
        L.ramx_xfam_candidates.restype = C.c_int64
        L.ramx_xfam_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(XfamLinkParams),
                                       C.c_void_p, C.c_void_p]
        L.ramx_xfam_groups.restype = C.c_int
        if hasattr(L, "ramx_cli_main"):
            L.ramx_cli_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        _lib = L
    return _lib


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise RamxError(f"{what} failed ({rc}): {lib().ramx_last_error().decode()}")
    return rc
