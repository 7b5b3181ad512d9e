"""ctypes binding of the C ABI in include/ntlink_amd.h (libntlink_hip.so).

The library is the hipcc-built HIP extension that sits next to this file.  There is no CPU
fallback: importing works anywhere (so that CLIs can print --help), but opening a Device without
the library or without a GPU raises.
"""
import ctypes as C
import threading
import weakref
import os

import numpy as np
from time import perf_counter as _now

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libntlink_hip.so")

# every symbol include/ntlink_amd.h declares
SYMBOLS = [
    "ntl_ctx_create", "ntl_ctx_destroy", "ntl_last_error", "ntl_ctx_device_name", "ntl_ctx_sync", "ntl_ctx_pipelined", "ntl_ctx_set_pipeline", "ntl_ctx_side_stream",
    "ntl_prof_enable", "ntl_prof_reset", "ntl_prof_get",
    "ntl_batch_create", "ntl_batch_create_packed", "ntl_batch_create_packed_at", "ntl_packed_words", "ntl_batch_destroy", "ntl_batch_nseq", "ntl_batch_bases", "ntl_host_alloc", "ntl_host_free",
    "ntl_synth_genome", "ntl_synth_slices", "ntl_batch_download", "ntl_batch_mask", "ntl_batch_download_n",
    "ntl_ascii_create", "ntl_ascii_destroy", "ntl_ascii_nrec", "ntl_ascii_bytes", "ntl_stitch", "ntl_stitched_bytes", "ntl_stitched_copy", "ntl_stitched_destroy",
    "ntl_stitched_base_counts",
    "ntl_sketch_run", "ntl_sketch_run_indexed", "ntl_sketch_run_for_map", "ntl_sketch_has_records", "ntl_sketch_destroy", "ntl_sketch_nseq", "ntl_sketch_count", "ntl_sketch_download",
    "ntl_sketch_strips", "ntl_sketch_redo_strips", "ntl_sketch_fallback_strips", "ntl_sketch_from_lists", "ntl_sketch_plan", "ntl_sketch_wait", "ntl_mapres_wait",
    "ntl_sketch_from_host", "ntl_overlap_filter", "ntl_overlap_cuts", "ntl_path_chains",
    "ntl_index_build", "ntl_index_destroy", "ntl_index_size",
    "ntl_map_run", "ntl_mapres_destroy", "ntl_mapres_n_mappings", "ntl_mapres_n_hits", "ntl_mapres_n_pafs",
    "ntl_mapres_n_index_hits", "ntl_mapres_download", "ntl_mapres_from_host", "ntl_mapres_liftover", "ntl_map_run_grouped", "ntl_mapres_grouped_info", "ntl_mapres_gap_cuts",
    "ntl_fastx_open", "ntl_fastx_open_range", "ntl_fastx_range", "ntl_fastx_close", "ntl_fastx_error", "ntl_fastx_next", "ntl_fastx_sizes", "ntl_fastx_copy", "ntl_fastx_copy_packed", "ntl_fastx_runs", "ntl_fastx_next_span", "ntl_fastx_parse_span", "ntl_fastx_copy_span", "ntl_fastx_seqs", "ntl_fastx_offsets",
    "ntl_fastx_names", "ntl_fastx_name_offsets", "ntl_write_indexlr", "ntl_write_verbose", "ntl_write_paf",
    "ntl_tsv_open", "ntl_tsv_close", "ntl_tsv_error", "ntl_tsv_next", "ntl_tsv_sizes", "ntl_tsv_copy",
    "ntl_vmap_open", "ntl_vmap_close", "ntl_vmap_error", "ntl_vmap_next", "ntl_vmap_sizes", "ntl_vmap_copy",
    "ntl_gap_pair_table", "ntl_gap_select", "ntl_gap_cands_count", "ntl_gap_cands_copy", "ntl_gap_cands_destroy",
    "ntl_tally_create", "ntl_tally_destroy", "ntl_tally_add", "ntl_tally_npairs", "ntl_tally_ngaps", "ntl_tally_export", "ntl_tally_merge",
    "ntl_liftover",
    "ntl_names_create", "ntl_names_destroy", "ntl_mapres_format", "ntl_text_sizes", "ntl_text_download", "ntl_text_destroy", "ntl_write_blob",
    "ntl_sketch_format", "ntl_sketch_text_limit", "ntl_sketch_text_bound", "ntl_sktext_bytes", "ntl_sktext_download", "ntl_sktext_destroy",
    "ntl_tally_add_ends", "ntl_tally_write", "ntl_io_errno",
    "ntl_pairtab_create", "ntl_pairtab_destroy", "ntl_mapres_pairs", "ntl_pairs_count", "ntl_pairs_download", "ntl_pairs_destroy", "ntl_tally_add_pairs",
]

MAPPING_DT = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("n_hits", "<u4"), ("pad", "<u4"), ("hit_off", "<u8")])
HIT_DT = np.dtype([("ctg_pos", "<u4"), ("read_pos", "<u4"), ("ctg_strand", "u1"), ("read_strand", "u1"),
                   ("pad", "u1", (2,))])
PAF_DT = np.dtype([("read", "<u4"), ("ctg", "<u4"), ("q_start", "<u4"), ("q_end", "<u4"),
                   ("t_start", "<u4"), ("t_end", "<u4"), ("n_hits", "<u4"), ("strand", "<u4")])
GAP_CUT_DT = np.dtype([(nm, "<u4") for nm in ("status", "src_ctg_pos", "src_read_cut", "src_end_cut", "tgt_ctg_pos", "tgt_read_cut",
                                               "tgt_end_cut", "ori")])  # ntl_gap_cut
NTL_GAP_NOT_TWO, NTL_GAP_SRC_MIXED_STRANDS, NTL_GAP_TGT_MIXED_STRANDS, NTL_GAP_SRC_POSITIONS, NTL_GAP_TGT_POSITIONS = 1, 2, 4, 8, 16
GAP_CAND_DT = np.dtype([(nm, "<u4") for nm in ("pair", "read", "anchors", "flags", "source_ctg_cut", "source_read_cut", "target_ctg_cut",
                                                "target_read_cut")])  # ntl_gap_cand
NTL_GAPSEL_VALID, NTL_GAPSEL_NEGATIVE, NTL_GAPSEL_VIA_REVCOMP = 1, 2, 4
STITCH_SEG_DT = np.dtype([(nm, "<u4") for nm in ("store", "rec", "lo", "hi", "flags")])  # ntl_stitch_seg
NTL_STITCH_FILL, NTL_STITCH_REVCOMP, NTL_STITCH_LOWER, NTL_STITCH_LOWER_FIRST = 0xFFFFFFFF, 1, 2, 4
OVERLAP_PAIR_DT = np.dtype([(nm, "<u4") for nm in ("src", "tgt", "src_start", "src_end", "tgt_start", "tgt_end", "src_len", "tgt_len", "signs",
                                                   "pad")])  # ntl_overlap_pair
OVERLAP_CUT_DT = np.dtype([(nm, "<u4") for nm in ("status", "n_shared", "n_comp", "src_cut", "tgt_cut", "pad")] + [("hash", "<u8")])  # ntl_overlap_cut
NTL_OVERLAP_CUT, NTL_OVERLAP_GLOBAL, NTL_OVERLAP_LDS_SLICE, NTL_OVERLAP_SRC_MINUS, NTL_OVERLAP_TGT_MINUS = 1, 2, 1024, 1, 2
PATH_EDGE_DT = np.dtype([("src", "<u4"), ("tgt", "<u4"), ("d", "<i4"), ("n", "<u4"), ("flags", "<u4")])  # ntl_path_edge
PATH_LINK_DT = np.dtype([("a", "<u4"), ("b", "<u4")])  # ntl_path_link
PATH_COUNTS_DT = np.dtype([(nm, "<u4") for nm in ("n_chain_vertices", "n_chains", "removed_linearize", "removed_transitive", "cycles")] +
                          [("reserved", "<u4", (3,))])  # ntl_path_counts
NTL_PATH_EDGE_NEW, NTL_PATH_CONSERVATIVE, NTL_PATH_STITCH, NTL_PATH_TRANSITIVE = 1, 0, 1, 2
LIFT_ENTRY_DT = np.dtype([(nm, "<u4") for nm in ("new_ctg", "mode", "scaf_start", "ctg_start", "ctg_end")])  # ntl_lift_entry
NTL_LIFT_ABSENT, NTL_LIFT_KEEP, NTL_LIFT_SHIFT, NTL_LIFT_MIRROR = 0, 1, 2, 3  # ntl_lift_entry.mode
NTL_LIFT_LANE_LINES = 16
PAIR_REC_DT = np.dtype([("src", "<u4"), ("tgt", "<u4"), ("gap", "<i8"), ("read", "<u4"), ("src_ori", "u1"), ("tgt_ori", "u1"), ("anchor", "u1"),
                        ("pad", "u1")])  # ntl_pair_rec
NTL_PAIR_LANE_MAPS = 16
NTL_SKETCH_TEXT_LEN, NTL_SKETCH_TEXT_STRAND = 1, 2  # flags of ntl_sketch_format
SKETCH_TEXT_PIECE = 256 << 20  # bound of one piece of Sketch.text: what the drain thread writes while the next piece is formatted
NO_CTG = 0xFFFFFFFF  # ntl_mapping.ctg of a name that is not in the reader's table


class MapParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("z", C.c_int32), ("x", C.c_double),
                ("sensitive", C.c_int32), ("repeat_filter", C.c_int32)]


class PlanInfo(C.Structure):
    """ntl_plan_info"""
    _fields_ = [(nm, C.c_int32) for nm in ("pass", "nt", "C", "NWO", "big", "direct", "wave_wavefronts", "wave_slots", "wave_rounds",
                                           "wave_kmers", "lists")] + [("thresh", C.c_uint32)]


class GroupedInfo(C.Structure):
    """ntl_grouped_info"""
    _fields_ = [("lds_slots", C.c_uint32), ("groups_in_lds", C.c_uint64), ("groups_in_global", C.c_uint64)]


PASSES = ("small", "exact_only", "block_minima", "thresh", "wave")  # NTL_PASS_*

NTL_EINVAL, NTL_EDEVICE, NTL_ENOMEM, NTL_EINTERNAL, NTL_ERANGE = -1, -2, -3, -4, -5


class NtlError(RuntimeError):
    pass


_libs = {}


def load(path=None):
    """dlopen the C-ABI library and declare its prototypes."""
    # NTLINK_AMD_LIB: another build of the same C ABI (the tests run the kernels' source under a CPU mock of the HIP runtime)
    path = path or os.environ.get("NTLINK_AMD_LIB") or DEFAULT_LIB
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise NtlError(f"HIP extension not built: {path} is missing (run __graft_entry__.build())")
    if path == DEFAULT_LIB and not os.environ.get("NTL_ALLOW_STALE_LIB"):
        # what runs is what the sources beside it say (build.py: content signatures; objects and library travel to the GPU box)
        from . import build
        if not build.library_is_current():
            raise NtlError(f"{path} was not built from the sources beside it (signature mismatch): run __graft_entry__.build()")
    L = C.CDLL(path)
    vp, u64p, u32p, u8p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    L.ntl_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.ntl_ctx_destroy.argtypes = [vp]
    L.ntl_ctx_destroy.restype = None
    L.ntl_last_error.argtypes = [vp]
    L.ntl_last_error.restype = C.c_char_p
    L.ntl_ctx_device_name.argtypes = [vp]
    L.ntl_ctx_device_name.restype = C.c_char_p
    L.ntl_ctx_sync.argtypes = [vp]
    L.ntl_ctx_pipelined.argtypes = [vp]
    L.ntl_ctx_set_pipeline.argtypes = [vp, C.c_int]
    L.ntl_ctx_side_stream.argtypes = [vp]
    L.ntl_sketch_wait.argtypes = [vp]
    L.ntl_mapres_wait.argtypes = [vp]
    L.ntl_prof_enable.argtypes = [vp, C.c_int]
    L.ntl_prof_reset.argtypes = [vp]
    L.ntl_prof_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), u64p]
    L.ntl_batch_create.argtypes = [vp, vp, u64p, C.c_uint64, C.POINTER(vp)]
    L.ntl_batch_create_packed.argtypes = [vp, vp, u64p, C.c_uint64, vp, vp, vp, C.c_uint64, C.POINTER(vp)]
    L.ntl_batch_create_packed_at.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.POINTER(vp)]
    L.ntl_fastx_next_span.argtypes = [vp, C.c_uint64, u64p, u64p]
    L.ntl_fastx_parse_span.argtypes = [vp, vp, u64p, u64p, u64p, u64p]
    L.ntl_fastx_copy_span.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64p]
    L.ntl_packed_words.argtypes = [C.c_uint64]
    L.ntl_packed_words.restype = C.c_uint64
    L.ntl_batch_destroy.argtypes = [vp]
    L.ntl_batch_destroy.restype = None
    L.ntl_batch_nseq.argtypes = [vp]
    L.ntl_batch_nseq.restype = C.c_uint64
    L.ntl_batch_bases.argtypes = [vp]
    L.ntl_batch_bases.restype = C.c_uint64
    L.ntl_synth_genome.argtypes = [vp, C.c_uint64, u32p, C.c_uint64, C.POINTER(vp)]
    L.ntl_synth_slices.argtypes = [vp, vp, C.c_uint64, C.c_uint64, u32p, u32p, u32p, u8p, C.c_double, C.c_double, C.c_double,
                                   C.POINTER(vp)]
    L.ntl_batch_download.argtypes = [vp, vp, u64p]
    L.ntl_batch_mask.argtypes = [vp, vp, C.c_uint64, u32p, u32p, u32p, C.POINTER(vp)]
    L.ntl_batch_download_n.argtypes = [vp, vp, u64p]
    L.ntl_ascii_create.argtypes = [vp, vp, u64p, C.c_uint64, C.POINTER(vp)]
    L.ntl_ascii_destroy.argtypes = [vp]
    L.ntl_ascii_destroy.restype = None
    for nm in ("ntl_ascii_nrec", "ntl_ascii_bytes", "ntl_stitched_bytes"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = C.c_uint64
    L.ntl_stitch.argtypes = [vp, C.POINTER(vp), C.c_uint32, vp, C.c_uint64, C.POINTER(vp)]
    L.ntl_stitched_copy.argtypes = [vp, C.c_uint64, C.c_uint64, vp]
    L.ntl_stitched_destroy.argtypes = [vp]
    L.ntl_stitched_destroy.restype = None
    L.ntl_stitched_base_counts.argtypes = [vp, u64p, C.c_uint64, u64p]
    L.ntl_sketch_run.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.ntl_sketch_run_indexed.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.ntl_sketch_run_for_map.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.ntl_sketch_has_records.argtypes = [vp]
    L.ntl_sketch_destroy.argtypes = [vp]
    L.ntl_sketch_destroy.restype = None
    L.ntl_sketch_nseq.argtypes = [vp]
    L.ntl_sketch_nseq.restype = C.c_uint64
    L.ntl_sketch_count.argtypes = [vp]
    L.ntl_sketch_count.restype = C.c_uint64
    for nm in ("ntl_sketch_strips", "ntl_sketch_redo_strips", "ntl_sketch_fallback_strips"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = C.c_uint64
    L.ntl_sketch_from_lists.argtypes = [vp]
    L.ntl_sketch_plan.argtypes = [vp, C.POINTER(PlanInfo)]
    L.ntl_sketch_download.argtypes = [vp, u64p, u64p, u32p, u8p]
    L.ntl_sketch_from_host.argtypes = [vp, C.c_uint64, u64p, u64p, u32p, u8p, C.POINTER(vp)]
    L.ntl_overlap_filter.argtypes = [vp, vp, u64p, u32p, u32p, C.POINTER(vp)]
    L.ntl_overlap_cuts.argtypes = [vp, vp, vp, C.c_uint64, vp]
    L.ntl_path_chains.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp]
    L.ntl_index_build.argtypes = [vp, vp, u32p, C.c_uint32, C.POINTER(vp)]
    L.ntl_index_destroy.argtypes = [vp]
    L.ntl_index_destroy.restype = None
    L.ntl_index_size.argtypes = [vp]
    L.ntl_index_size.restype = C.c_uint64
    L.ntl_map_run.argtypes = [vp, vp, vp, u32p, C.POINTER(MapParams), C.POINTER(vp)]
    L.ntl_map_run_grouped.argtypes = [vp, vp, u32p, u32p, vp, u32p, u32p, C.c_uint32, C.POINTER(MapParams), C.POINTER(vp)]
    L.ntl_mapres_grouped_info.argtypes = [vp, C.POINTER(GroupedInfo)]
    L.ntl_mapres_gap_cuts.argtypes = [vp, vp, vp, C.c_uint32, C.c_int32, vp]
    L.ntl_mapres_destroy.argtypes = [vp]
    L.ntl_mapres_destroy.restype = None
    for nm in ("n_mappings", "n_hits", "n_pafs", "n_index_hits"):
        f = getattr(L, "ntl_mapres_" + nm)
        f.argtypes = [vp]
        f.restype = C.c_uint64
    L.ntl_mapres_download.argtypes = [vp, vp, vp, vp]
    L.ntl_mapres_from_host.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(vp)]
    L.ntl_mapres_liftover.argtypes = [vp, vp, vp, C.c_uint32, C.c_int32, C.POINTER(vp)]
    L.ntl_host_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.ntl_host_free.argtypes = [vp, vp]
    L.ntl_host_free.restype = None
    L.ntl_fastx_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.ntl_fastx_open_range.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.ntl_fastx_range.argtypes = [vp, u64p, u64p]
    L.ntl_fastx_range.restype = None
    L.ntl_fastx_close.argtypes = [vp]
    L.ntl_fastx_close.restype = None
    L.ntl_fastx_error.argtypes = [vp]
    L.ntl_fastx_error.restype = C.c_char_p
    L.ntl_fastx_next.argtypes = [vp, C.c_uint64, u64p]
    L.ntl_fastx_sizes.argtypes = [vp, u64p, u64p, u64p]
    L.ntl_fastx_sizes.restype = None
    L.ntl_fastx_copy.argtypes = [vp, vp, vp, vp, vp]
    L.ntl_fastx_copy_packed.argtypes = [vp, vp, vp, vp, vp, u64p]
    L.ntl_fastx_runs.argtypes = [vp, vp, vp, vp]
    for nm in ("seqs", "offsets", "names", "name_offsets"):
        f = getattr(L, "ntl_fastx_" + nm)
        f.argtypes = [vp]
        f.restype = vp
    L.ntl_write_indexlr.argtypes = [C.c_int, C.c_uint64, vp, u64p, u32p, u64p, u64p, u32p, u8p]
    L.ntl_write_verbose.argtypes = [C.c_int, vp, C.c_uint64, vp, vp, u64p, vp, u64p]
    L.ntl_write_paf.argtypes = [C.c_int, vp, C.c_uint64, vp, u64p, u32p, vp, u64p, u32p]
    L.ntl_tsv_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.ntl_tsv_close.argtypes = [vp]
    L.ntl_tsv_close.restype = None
    L.ntl_tsv_error.argtypes = [vp]
    L.ntl_tsv_error.restype = C.c_char_p
    L.ntl_tsv_next.argtypes = [vp, C.c_uint64, u64p]
    L.ntl_tsv_sizes.argtypes = [vp, u64p, u64p, u64p]
    L.ntl_tsv_sizes.restype = None
    L.ntl_tsv_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ntl_vmap_open.argtypes = [C.c_char_p, vp, u64p, C.c_uint64, C.POINTER(vp)]
    L.ntl_vmap_close.argtypes = [vp]
    L.ntl_vmap_close.restype = None
    L.ntl_vmap_error.argtypes = [vp]
    L.ntl_vmap_error.restype = C.c_char_p
    L.ntl_vmap_next.argtypes = [vp, C.c_uint64, u64p]
    L.ntl_vmap_sizes.argtypes = [vp, u64p, u64p, u64p, u64p]
    L.ntl_vmap_sizes.restype = None
    L.ntl_vmap_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ntl_gap_pair_table.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint64]
    L.ntl_gap_select.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, vp, C.c_uint64, C.POINTER(vp)]
    L.ntl_gap_cands_count.argtypes = [vp]
    L.ntl_gap_cands_count.restype = C.c_uint64
    L.ntl_gap_cands_copy.argtypes = [vp, vp]
    L.ntl_gap_cands_destroy.argtypes = [vp]
    L.ntl_gap_cands_destroy.restype = None
    L.ntl_tally_create.argtypes = [vp, u64p, u32p, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp)]
    L.ntl_tally_destroy.argtypes = [vp]
    L.ntl_tally_destroy.restype = None
    L.ntl_tally_add.argtypes = [vp, vp, C.c_uint64, vp, u32p]
    L.ntl_tally_add_ends.argtypes = [vp, vp, C.c_uint64, vp, u32p]
    L.ntl_tally_add_pairs.argtypes = [vp, vp, C.c_uint64]
    L.ntl_pairtab_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.ntl_pairtab_destroy.argtypes = [vp]
    L.ntl_pairtab_destroy.restype = None
    L.ntl_mapres_pairs.argtypes = [vp, vp, u32p, C.c_uint64, C.POINTER(vp)]
    L.ntl_pairs_count.argtypes = [vp]
    L.ntl_pairs_count.restype = C.c_uint64
    L.ntl_pairs_download.argtypes = [vp, vp]
    L.ntl_pairs_destroy.argtypes = [vp]
    L.ntl_pairs_destroy.restype = None
    L.ntl_names_create.argtypes = [vp, vp, u64p, u32p, C.c_uint64, C.POINTER(vp)]
    L.ntl_names_destroy.argtypes = [vp]
    L.ntl_names_destroy.restype = None
    L.ntl_mapres_format.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.ntl_text_sizes.argtypes = [vp, u64p, u64p, u64p]
    L.ntl_text_sizes.restype = None
    L.ntl_text_download.argtypes = [vp, vp, vp, vp, vp]
    L.ntl_text_destroy.argtypes = [vp]
    L.ntl_text_destroy.restype = None
    L.ntl_write_blob.argtypes = [C.c_int, vp, C.c_uint64]
    L.ntl_sketch_format.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    L.ntl_sketch_text_limit.argtypes = []
    L.ntl_sketch_text_limit.restype = C.c_uint64
    L.ntl_sketch_text_bound.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.ntl_sketch_text_bound.restype = C.c_uint64
    L.ntl_sktext_bytes.argtypes = [vp]
    L.ntl_sktext_bytes.restype = C.c_uint64
    L.ntl_sktext_download.argtypes = [vp, vp]
    L.ntl_sktext_destroy.argtypes = [vp]
    L.ntl_sktext_destroy.restype = None
    for nm in ("npairs", "ngaps"):
        f = getattr(L, "ntl_tally_" + nm)
        f.argtypes = [vp]
        f.restype = C.c_uint64
    L.ntl_tally_export.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ntl_tally_write.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_char_p, u64p]
    L.ntl_io_errno.argtypes = []
    L.ntl_tally_merge.argtypes = [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    L.ntl_liftover.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, vp, u64p, vp, u64p, vp, vp, vp, vp, u64p, u64p]
    _libs[path] = L
    return L


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class _Handle:
    _destroy = None

    def __init__(self, dev, ptr):
        self.dev, self.ptr = dev, ptr
        dev._live.add(self)  # closed with the device at the latest

    def close(self):
        if self.ptr:
            if self.dev.ptr:  # a handle that outlives its context (interpreter shutdown order) must not touch it any more
                getattr(self.dev.L, self._destroy)(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Batch(_Handle):
    """Sequences resident in HBM as packed 2-bit bases + ACGT-run table."""
    _destroy = "ntl_batch_destroy"

    @property
    def nseq(self):
        return int(self.dev.L.ntl_batch_nseq(self.ptr))

    @property
    def bases(self):
        return int(self.dev.L.ntl_batch_bases(self.ptr))

    def download(self):
        """(ASCII bases uint8, offsets u64[nseq+1]) of a pure-ACGT batch (the synthetic ones)."""
        buf = np.empty(max(self.bases, 1), np.uint8)
        off = np.zeros(self.nseq + 1, np.uint64)
        self.dev._chk(self.dev.L.ntl_batch_download(self.ptr, buf.ctypes.data, _ptr(off, C.c_uint64)))
        return buf[:self.bases], off

    def download_n(self):
        """(ASCII bases uint8, offsets u64[nseq+1]) of any batch (ntl_batch_download_n): upper case, N wherever no ACGT run covers a
        base -- a masked stretch, an N or an IUPAC code of the input."""
        off = np.zeros(self.nseq + 1, np.uint64)
        buf = np.empty(max(self.bases, 1), np.uint8)
        self.dev._chk(self.dev.L.ntl_batch_download_n(self.ptr, buf.ctypes.data, _ptr(off, C.c_uint64)))
        return buf[:int(off[-1])], off


class Ascii(_Handle):
    """Records resident on the device as the bytes they were read as (ntl_ascii): the sources of Device.stitch."""
    _destroy = "ntl_ascii_destroy"

    @property
    def nrec(self):
        return int(self.dev.L.ntl_ascii_nrec(self.ptr))

    @property
    def nbytes(self):
        return int(self.dev.L.ntl_ascii_bytes(self.ptr))


class Stitched(_Handle):
    """The text Device.stitch assembled, on the device until it is copied."""
    _destroy = "ntl_stitched_destroy"

    @property
    def nbytes(self):
        return int(self.dev.L.ntl_stitched_bytes(self.ptr))

    def copy(self, lo, hi, out):
        """bytes [lo, hi) into the uint8 array `out` (Device.pinned_empty: one DMA); waits for the device"""
        if len(out) < hi - lo:
            raise ValueError("the destination is smaller than the range")
        self.dev._chk(self.dev.L.ntl_stitched_copy(self.ptr, int(lo), int(hi), out.ctypes.data))
        return out[:hi - lo]

    def download(self):
        """the whole text as a uint8 array"""
        n = self.nbytes
        return self.copy(0, n, np.empty(max(n, 1), np.uint8))[:n]

    def base_counts(self, rec_off):
        """Called bases per record (ntl_stitched_base_counts, csrc/count_kernels.h): rec_off = n + 1 ascending offsets into the text
        -> u64[n], the bytes of [rec_off[i], rec_off[i + 1]) that are one of ACGTacgt.  Waits for the device."""
        off = np.ascontiguousarray(rec_off, np.uint64)
        if off.ndim != 1:
            raise ValueError("rec_off must be one-dimensional")
        n = max(len(off) - 1, 0)
        out = np.zeros(n, np.uint64)
        self.dev._chk(self.dev.L.ntl_stitched_base_counts(self.ptr, _ptr(off, C.c_uint64), n, _ptr(out, C.c_uint64)))
        return out


class Sketch(_Handle):
    """Device-resident minimizer lists (the output of `indexlr --long --pos --strand`)."""
    _destroy = "ntl_sketch_destroy"

    @property
    def nseq(self):
        return int(self.dev.L.ntl_sketch_nseq(self.ptr))

    def wait(self):
        """Block until the device has finished this sketch (the calls that make one only queue work)."""
        self.dev._chk(self.dev.L.ntl_sketch_wait(self.ptr))
        return self

    @property
    def count(self):
        self.wait()
        return int(self.dev.L.ntl_sketch_count(self.ptr))

    @property
    def strips(self):
        return int(self.dev.L.ntl_sketch_strips(self.ptr))

    @property
    def redo_strips(self):
        self.wait()
        return int(self.dev.L.ntl_sketch_redo_strips(self.ptr))

    @property
    def fallback_strips(self):
        self.wait()
        return int(self.dev.L.ntl_sketch_fallback_strips(self.ptr))

    @property
    def has_records(self):
        """False for a sketch made only to be mapped (Device.sketch(..., index=ix, records=False)): nothing to download."""
        return bool(self.dev.L.ntl_sketch_has_records(self.ptr))

    @property
    def from_lists(self):
        """True: the window passes wrote per-strip minimizer lists; False: the bitmask (diagnostics; same result)."""
        self.wait()
        return bool(self.dev.L.ntl_sketch_from_lists(self.ptr))

    @property
    def plan(self):
        """The window pass the sketch ran (ntl_sketch_plan; diagnostics): dict(pass= one of PASSES, nt=, C=, NWO=, big=, direct=,
        shape= sketch_wave_kernel's (wavefronts per workgroup, slots per lane, scan rounds, k-mers per lane) or None, lists=, thresh=)."""
        info = PlanInfo()
        self.dev._chk(self.dev.L.ntl_sketch_plan(self.ptr, C.byref(info)))
        wave = PASSES[getattr(info, "pass")] == "wave"
        return {"pass": PASSES[getattr(info, "pass")], "nt": info.nt, "C": info.C, "NWO": info.NWO, "big": bool(info.big),
                "direct": bool(info.direct),
                "shape": (info.wave_wavefronts, info.wave_slots, info.wave_rounds, info.wave_kmers) if wave else None,
                "lists": bool(info.lists), "thresh": info.thresh}

    def download(self):
        """(mx_off u64[nseq+1], hash u64, pos u32, strand u8 [1 = '+'])."""
        n, ns = self.count, self.nseq
        off = np.zeros(ns + 1, np.uint64)
        h = np.empty(n, np.uint64); p = np.empty(n, np.uint32); s = np.empty(n, np.uint8)
        self.dev._chk(self.dev.L.ntl_sketch_download(self.ptr, _ptr(off, C.c_uint64), _ptr(h, C.c_uint64),
                                                     _ptr(p, C.c_uint32), _ptr(s, C.c_uint8)))
        return off, h, p, s

    def offsets(self):
        """mx_off u64[nseq+1] alone (no record crosses PCIe)."""
        self.wait()
        off = np.zeros(self.nseq + 1, np.uint64)
        self.dev._chk(self.dev.L.ntl_sketch_download(self.ptr, _ptr(off, C.c_uint64), None, None, None))
        return off

    def format(self, names, with_len, with_strand=True, seq_lo=0, seq_hi=None):
        """The lines of the sequences [seq_lo, seq_hi) of indexlr's TSV, made on the device (ntl_sketch_format): one call, one
        SketchText.  names: the NameTable (Device.names) of the batch's names and lengths.  NtlError with .code NTL_ERANGE where
        the range's bound reaches the limit of one call: Sketch.text cuts."""
        flags = (NTL_SKETCH_TEXT_LEN if with_len else 0) | (NTL_SKETCH_TEXT_STRAND if with_strand else 0)
        p = C.c_void_p()
        self.dev._chk(self.dev.L.ntl_sketch_format(self.ptr, names.ptr, flags, int(seq_lo), int(self.nseq if seq_hi is None else seq_hi), C.byref(p)))
        return SketchText(self.dev, p)

    def text_ranges(self, names, piece_bytes=None):
        """The ranges [lo, hi) Sketch.text formats, in order -- the one place where a sketch is cut: each the longest run of whole
        sequences whose bound (ntl_sketch_text_bound: 34 bytes per minimizer, the longest name + 13 per sequence) stays below the
        limit of one call (ntl_sketch_text_limit) and below piece_bytes (default SKETCH_TEXT_PIECE).  A sequence that alone reaches
        the limit is a range of its own: the call refuses it (NTL_ERANGE), it is not split."""
        L = self.dev.L
        limit = min(int(L.ntl_sketch_text_limit()), int(SKETCH_TEXT_PIECE if piece_bytes is None else piece_bytes))
        per_seq, per_mx = int(L.ntl_sketch_text_bound(names.ptr, 1, 0)), int(L.ntl_sketch_text_bound(names.ptr, 0, 1))
        nseq = self.nseq
        cum = self.offsets().astype(np.int64) * per_mx + np.arange(nseq + 1, dtype=np.int64) * per_seq  # the bound of [0, i)
        out, lo = [], 0
        while lo < nseq:
            hi = int(np.searchsorted(cum, cum[lo] + limit, side="left")) - 1  # the last hi with cum[hi] - cum[lo] < limit
            hi = max(hi, lo + 1)
            out.append((lo, hi))
            lo = hi
        return out

    def text(self, names, with_len, with_strand=True, piece_bytes=None):
        """indexlr's TSV of this sketch, made on the device: yields its pieces in sequence order, each a uint8 array in page-locked
        memory of the device's pool (hand it to Device.pinned_release() when it has been written).  No record is downloaded."""
        for lo, hi in self.text_ranges(names, piece_bytes):
            with self.format(names, with_len, with_strand, lo, hi) as t:
                yield t.download()


class SketchText(_Handle):
    """Lines of indexlr's TSV of one range of a sketch's sequences, formatted on the device."""
    _destroy = "ntl_sktext_destroy"

    @property
    def nbytes(self):
        return int(self.dev.L.ntl_sktext_bytes(self.ptr))

    def download(self):
        """The bytes as a uint8 array in a page-locked buffer of the device's pool (Device.pinned_release() gives it back)."""
        buf = self.dev.pinned_empty(self.nbytes)
        self.dev._chk(self.dev.L.ntl_sktext_download(self.ptr, buf.ctypes.data if len(buf) else None))
        return buf


class Index(_Handle):
    """Contig minimizer -> (contig, position, strand), duplicates removed."""
    _destroy = "ntl_index_destroy"

    def __len__(self):
        return int(self.dev.L.ntl_index_size(self.ptr))


class MapResult(_Handle):
    _destroy = "ntl_mapres_destroy"

    def wait(self):
        """Block until the device has finished this result (Device.map only queues work)."""
        self.dev._chk(self.dev.L.ntl_mapres_wait(self.ptr))
        return self

    @property
    def n_index_hits(self):
        self.wait()
        return int(self.dev.L.ntl_mapres_n_index_hits(self.ptr))

    @property
    def grouped_info(self):
        """Of a result of Device.map_grouped (ntl_mapres_grouped_info; diagnostics): dict(lds_slots=, groups_in_lds=, groups_in_global=)
        -- where the groups' tables lived.  An ordinary result raises."""
        info = GroupedInfo()
        self.dev._chk(self.dev.L.ntl_mapres_grouped_info(self.ptr, C.byref(info)))
        return {"lds_slots": int(info.lds_slots), "groups_in_lds": int(info.groups_in_lds), "groups_in_global": int(info.groups_in_global)}

    def gap_cuts(self, src_minus, tgt_minus, k):
        """Of a result of Device.map_grouped whose group g is contigs 2g, 2g + 1 and read g (ntl_mapres_gap_cuts): one GAP_CUT_DT
        record per gap -- status (0: valid, else NTL_GAP_* bits and zeros), the terminal minimizers' contig positions, the read cuts,
        the scaffold end cuts and the read-based orientations -- decided on the device from the hits where they lie.  src_minus /
        tgt_minus: per gap, true where the node's sign in the path is '-'; k: the k of this mapping.  The result may be pending."""
        sm = np.ascontiguousarray(src_minus, np.uint8); tm = np.ascontiguousarray(tgt_minus, np.uint8)
        if sm.ndim != 1 or sm.shape != tm.shape:
            raise ValueError("src_minus and tgt_minus must have one entry per gap each")
        out = np.empty(len(sm), GAP_CUT_DT)
        self.dev._chk(self.dev.L.ntl_mapres_gap_cuts(self.ptr, sm.ctypes.data, tm.ctypes.data, len(sm), int(k), out.ctypes.data))
        return out

    def counts(self):
        self.wait()
        L = self.dev.L
        return (int(L.ntl_mapres_n_mappings(self.ptr)), int(L.ntl_mapres_n_hits(self.ptr)),
                int(L.ntl_mapres_n_pafs(self.ptr)))

    def download(self, pinned=False):
        """dict(maps=, hits=, pafs=) of structured arrays, read order.  pinned=True puts them in one
        page-locked buffer of the device's pool (a single fast DMA instead of staged copies into fresh
        pages); hand dict["_pinned"] to Device.pinned_release() when the records have been consumed."""
        nm, nh, npf = self.counts()
        if pinned:
            sizes = [nm * MAPPING_DT.itemsize, nh * HIT_DT.itemsize, npf * PAF_DT.itemsize]
            offs = [0, (sizes[0] + 63) & ~63, 0]
            offs[2] = (offs[1] + sizes[1] + 63) & ~63
            base = self.dev.pinned_empty(offs[2] + sizes[2] + 64)
            maps = base[offs[0]:offs[0] + sizes[0]].view(MAPPING_DT)
            hits = base[offs[1]:offs[1] + sizes[1]].view(HIT_DT)
            pafs = base[offs[2]:offs[2] + sizes[2]].view(PAF_DT)
            self.dev._chk(self.dev.L.ntl_mapres_download(self.ptr, maps.ctypes.data, hits.ctypes.data, pafs.ctypes.data))
            return {"maps": maps, "hits": hits, "pafs": pafs, "_pinned": base, "_owner": self.dev}
        maps = np.empty(nm, MAPPING_DT); hits = np.empty(nh, HIT_DT); pafs = np.empty(npf, PAF_DT)
        self.dev._chk(self.dev.L.ntl_mapres_download(self.ptr, maps.ctypes.data, hits.ctypes.data, pafs.ctypes.data))
        return {"maps": maps, "hits": hits, "pafs": pafs}

    def format(self, read_names, ctg_names, verbose=True, paf=True):
        """The text of this result's lines, made on the device (ntl_mapres_format): read_names / ctg_names are NameTables
        (Device.names) with lengths.  The result must stay open until the Text has been downloaded."""
        p = C.c_void_p()
        self.dev._chk(self.dev.L.ntl_mapres_format(self.ptr, read_names.ptr, ctg_names.ptr, int(bool(verbose)), int(bool(paf)), C.byref(p)))
        return Text(self.dev, p)


class NameTable(_Handle):
    """A name table (+ sequence lengths) resident on the device: the strings the text kernels copy into their lines."""
    _destroy = "ntl_names_destroy"


class PairTable(_Handle):
    """What the pair rules need of a tally, resident on the device (ntl_pairtab): name rank and length per contig, k and f."""
    _destroy = "ntl_pairtab_destroy"


class Text(_Handle):
    """The lines of .verbose_mapping.tsv / .paf of one map result, formatted on the device."""
    _destroy = "ntl_text_destroy"

    def sizes(self):
        v, p, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.dev.L.ntl_text_sizes(self.ptr, C.byref(v), C.byref(p), C.byref(n))
        return int(v.value), int(p.value), int(n.value)

    def download(self):
        """dict(verbose=bytes as uint8, paf=..., maps=, ends= [2 per mapping: first and last hit]) in ONE page-locked buffer of
        the device's pool; hand dict["_pinned"] to Device.pinned_release() when it has been written out."""
        nv, npf, nm = self.sizes()
        sizes = [nv, npf, nm * MAPPING_DT.itemsize, 2 * nm * HIT_DT.itemsize]
        offs, at = [], 0
        for sz in sizes:
            offs.append(at)
            at = (at + sz + 63) & ~63
        base = self.dev.pinned_empty(at + 64)
        verbose = base[offs[0]:offs[0] + nv]
        paf = base[offs[1]:offs[1] + npf]
        maps = base[offs[2]:offs[2] + sizes[2]].view(MAPPING_DT)
        ends = base[offs[3]:offs[3] + sizes[3]].view(HIT_DT)
        self.dev._chk(self.dev.L.ntl_text_download(self.ptr, verbose.ctypes.data, paf.ctypes.data, maps.ctypes.data, ends.ctypes.data))
        return {"verbose": verbose, "paf": paf, "maps": maps, "ends": ends, "_pinned": base, "_owner": self.dev}


class Device:
    """One MI355X: context + stream.  Raises NtlError when there is no GPU or no HIP extension."""

    def __init__(self, device=0, lib_path=None):
        self.L = load(lib_path)
        self.ordinal, self.lib_path = int(device), lib_path
        p = C.c_void_p()
        rc = self.L.ntl_ctx_create(int(device), C.byref(p))
        if rc != 0:
            raise NtlError(f"ntl_ctx_create(device={device}) failed with {rc}: no usable GPU "
                           f"(this package has no CPU path)")
        self.ptr = p
        self._live = weakref.WeakSet()
        self._pinned_free, self._pinned_all, self._pinned_out = [], [], {}  # (address, capacity) of page-locked buffers
        self._pinned_lock = threading.Lock()  # the reader thread takes buffers, the device thread returns them
        self.pin_alloc_s, self.pin_alloc_bytes, self.pin_alloc_caps = 0.0, 0, []

    def workers(self, n):
        """n - 1 further contexts on the same GPU, kept for the life of this Device: the pair driver's device workers.  Their block
        caches and page-locked result buffers survive from one run_pair call to the next."""
        pool = self.__dict__.setdefault("_workers", [])
        while len(pool) < n - 1:
            pool.append(self.clone())
        return pool[:max(0, n - 1)]

    def clone(self):
        """Another context (stream, block cache, staging pool) on the same GPU: a second worker thread of the pair driver
        uploads its batch while this one's kernels run.  Device objects of one context may be used by the other."""
        return Device(self.ordinal, self.lib_path)

    def close(self):
        if self.ptr:
            for wk in self.__dict__.pop("_workers", []):
                wk.close()
            for h in list(self._live):  # device objects die before their context
                h.close()
            for addr, _cap in self._pinned_all:
                self.L.ntl_host_free(self.ptr, addr)
            self._pinned_free, self._pinned_all, self._pinned_out = [], [], {}
            self.L.ntl_ctx_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            exc = NtlError(f"error {rc}: {self.L.ntl_last_error(self.ptr).decode()}")
            exc.code = rc
            raise exc

    @property
    def name(self):
        return self.L.ntl_ctx_device_name(self.ptr).decode()

    def sync(self):
        self._chk(self.L.ntl_ctx_sync(self.ptr))

    @property
    def pipelined(self):
        return bool(self.L.ntl_ctx_pipelined(self.ptr))

    @property
    def side_stream(self):
        """The window stage's give-up passes run on a third stream (pipelined contexts made under NTL_SIDE_STREAM=1 or 2)."""
        return bool(self.L.ntl_ctx_side_stream(self.ptr))

    def set_pipeline(self, on):
        """Window stage on its own stream (on) or behind everything else on the one stream (off); drains the device first."""
        self._chk(self.L.ntl_ctx_set_pipeline(self.ptr, int(bool(on))))

    # ---- profiling (HIP events on the context's stream)
    def prof_enable(self, on=True):
        self._chk(self.L.ntl_prof_enable(self.ptr, int(on)))

    def prof_reset(self):
        self._chk(self.L.ntl_prof_reset(self.ptr))

    def prof_get(self, name):
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self.L.ntl_prof_get(self.ptr, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    # ---- page-locked staging buffers for sequence bytes
    def pinned_empty(self, nbytes):
        """uint8 array of nbytes in page-locked memory from a small pool (reused buffers are already
        faulted in, and their copy to the device is one DMA).  Give it back with pinned_release();
        the memory is only valid while this Device is open."""
        nbytes = int(nbytes)
        with self._pinned_lock:
            pick = None
            for i, (addr, cap) in enumerate(self._pinned_free):
                if nbytes <= cap <= 4 * nbytes + (1 << 20) and (pick is None or cap < self._pinned_free[pick][1]):
                    pick = i
            if pick is None:
                cap = max(int(nbytes * 1.125) + 4096, 1 << 20)
                p = C.c_void_p()
                t0 = _now()
                self._chk(self.L.ntl_host_alloc(self.ptr, cap, C.byref(p)))
                self.pin_alloc_s += _now() - t0  # page-locking is the expensive part of a process's first pass
                self.pin_alloc_bytes += cap
                self.pin_alloc_caps.append(cap)
                addr = p.value
                self._pinned_all.append((addr, cap))
            else:
                addr, cap = self._pinned_free.pop(pick)
            self._pinned_out[addr] = (addr, cap)
        return np.frombuffer((C.c_uint8 * cap).from_address(addr), np.uint8)[:nbytes]

    def pinned_release(self, arr):
        """No-op for arrays that did not come from pinned_empty()."""
        if arr is None:
            return
        with self._pinned_lock:
            ent = self._pinned_out.pop(arr.ctypes.data, None)
            if ent is not None:
                self._pinned_free.append(ent)

    # ---- the path
    def batch(self, seqs, offsets=None):
        """seqs: list of bytes, or one contiguous bytes/uint8 buffer with offsets[n+1]."""
        if offsets is None:
            lens = np.fromiter((len(s) for s in seqs), np.uint64, len(seqs))
            offsets = np.zeros(len(seqs) + 1, np.uint64)
            np.cumsum(lens, out=offsets[1:])
            buf = np.frombuffer(b"".join(seqs), np.uint8)
        else:
            buf = seqs if isinstance(seqs, np.ndarray) else np.frombuffer(seqs, np.uint8)
            offsets = np.ascontiguousarray(offsets, np.uint64)
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        p = C.c_void_p()
        self._chk(self.L.ntl_batch_create(self.ptr, buf.ctypes.data, _ptr(offsets, C.c_uint64), len(offsets) - 1,
                                          C.byref(p)))
        return Batch(self, p)

    def batch_packed(self, ss):
        """A SeqSet read with packed=True (seqio.load): 2-bit bases + ACGT-run table made by the parser threads."""
        p = C.c_void_p()
        if ss.positions is not None:  # read in one pass: the sequences of a parser thread sit at an upper bound of their place
            lens = ss.lengths
            self._chk(self.L.ntl_batch_create_packed_at(self.ptr, ss.packed.ctypes.data, int(ss.span_positions), ss.positions.ctypes.data,
                                                        lens.ctypes.data, len(lens), ss.seq_run_first.ctypes.data, ss.run_start.ctypes.data,
                                                        ss.run_len.ctypes.data, len(ss.run_start), C.byref(p)))
            return Batch(self, p)
        self._chk(self.L.ntl_batch_create_packed(self.ptr, ss.packed.ctypes.data, _ptr(ss.offsets, C.c_uint64), len(ss.offsets) - 1,
                                                 ss.seq_run_first.ctypes.data, ss.run_start.ctypes.data, ss.run_len.ctypes.data,
                                                 len(ss.run_start), C.byref(p)))
        return Batch(self, p)

    def synth_genome(self, seed, lengths):
        """Uniform random ACGT sequences generated on the device (bench / test support)."""
        ln = np.ascontiguousarray(lengths, np.uint32)
        p = C.c_void_p()
        self._chk(self.L.ntl_synth_genome(self.ptr, int(seed), _ptr(ln, C.c_uint32), len(ln), C.byref(p)))
        return Batch(self, p)

    def synth_slices(self, src, seed, src_seq, src_start, out_len, reverse=None, sub=0.0, ins=0.0, dele=0.0):
        """Slices of the sequences of batch `src` (reverse-complemented where reverse[i]), with per-base
        error events: contigs cut from chromosomes (no errors), reads sampled from them (with errors)."""
        sq = np.ascontiguousarray(src_seq, np.uint32); st = np.ascontiguousarray(src_start, np.uint32)
        ln = np.ascontiguousarray(out_len, np.uint32)
        rv = None if reverse is None else np.ascontiguousarray(reverse, np.uint8)
        if not (len(sq) == len(st) == len(ln)) or (rv is not None and len(rv) != len(ln)):
            raise ValueError("slice arrays must have one entry per output sequence")
        p = C.c_void_p()
        self._chk(self.L.ntl_synth_slices(self.ptr, src.ptr, int(seed), len(ln), _ptr(sq, C.c_uint32), _ptr(st, C.c_uint32),
                                          _ptr(ln, C.c_uint32), None if rv is None else _ptr(rv, C.c_uint8),
                                          float(sub), float(ins), float(dele), C.byref(p)))
        return Batch(self, p)

    def batch_mask(self, src, src_seq, keep_lo, keep_hi):
        """N-masked full-length copies of records of the resident batch `src` (ntl_batch_mask, csrc/mask_kernels.h): record i of the
        result is record src_seq[i] with every base outside [keep_lo[i], keep_hi[i]) replaced by N -- what the reference's
        print_masked_sequences writes to its temporary files, made where the bases already are.  Positions stay in the source
        record's coordinates.  The call waits for the device; the arrays and `src` may go once it returns."""
        sq = np.ascontiguousarray(src_seq, np.uint32); lo = np.ascontiguousarray(keep_lo, np.uint32)
        hi = np.ascontiguousarray(keep_hi, np.uint32)
        if sq.ndim != 1 or not (sq.shape == lo.shape == hi.shape):
            raise ValueError("src_seq, keep_lo and keep_hi must have one entry per output record each")
        p = C.c_void_p()
        self._chk(self.L.ntl_batch_mask(self.ptr, src.ptr, len(sq), _ptr(sq, C.c_uint32), _ptr(lo, C.c_uint32), _ptr(hi, C.c_uint32),
                                        C.byref(p)))
        return Batch(self, p)

    def ascii(self, seqs, offsets=None):
        """Records resident as they are (ntl_ascii_create): seqs as Device.batch takes them -- a list of bytes, or one contiguous
        bytes / uint8 buffer with offsets[n+1]."""
        if offsets is None:
            lens = np.fromiter((len(s) for s in seqs), np.uint64, len(seqs))
            offsets = np.zeros(len(seqs) + 1, np.uint64)
            np.cumsum(lens, out=offsets[1:])
            buf = np.frombuffer(b"".join(seqs), np.uint8)
        else:
            buf = seqs if isinstance(seqs, np.ndarray) else np.frombuffer(seqs, np.uint8)
            offsets = np.ascontiguousarray(offsets, np.uint64)
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        p = C.c_void_p()
        self._chk(self.L.ntl_ascii_create(self.ptr, buf.ctypes.data, _ptr(offsets, C.c_uint64), len(offsets) - 1, C.byref(p)))
        return Ascii(self, p)

    def stitch(self, stores, segs):
        """The concatenation of the segments (ntl_stitch, csrc/stitch_kernels.h): stores = a list of Ascii, segs = STITCH_SEG_DT
        records (or tuples) {store, rec, lo, hi, flags} -- bytes [lo, hi) of record rec of stores[store], reverse-complemented
        (NTL_STITCH_REVCOMP), lower-cased (NTL_STITCH_LOWER) or with the first output byte lower-cased (NTL_STITCH_LOWER_FIRST);
        store NTL_STITCH_FILL: hi - lo copies of the byte `rec`.  Only queues; -> Stitched."""
        sg = np.ascontiguousarray(segs if isinstance(segs, np.ndarray) else np.array(list(segs), STITCH_SEG_DT), STITCH_SEG_DT)
        if sg.ndim != 1:
            raise ValueError("segs must be one-dimensional")
        ptrs = (C.c_void_p * max(len(stores), 1))(*[st.ptr for st in stores])
        p = C.c_void_p()
        self._chk(self.L.ntl_stitch(self.ptr, ptrs, len(stores), sg.ctypes.data if len(sg) else None, len(sg), C.byref(p)))
        return Stitched(self, p)

    def sketch(self, batch, k, w, index=None, records=True):
        """index: the contig Index the sketch will be mapped against -- its minimizers are then looked up while they are emitted
        and Device.map(index, sketch, ...) skips its lookup pass (same records either way).  records=False (with an index): the
        sketch is made only for that map (ntl_sketch_run_for_map): no records to download."""
        p = C.c_void_p()
        if index is None:
            self._chk(self.L.ntl_sketch_run(self.ptr, batch.ptr, int(k), int(w), C.byref(p)))
        elif not records:
            self._chk(self.L.ntl_sketch_run_for_map(self.ptr, batch.ptr, int(k), int(w), index.ptr, C.byref(p)))
        else:
            self._chk(self.L.ntl_sketch_run_indexed(self.ptr, batch.ptr, int(k), int(w), index.ptr, C.byref(p)))
        return Sketch(self, p)

    def sketch_from_arrays(self, mx_off, mx_hash, pos, strand):
        mx_off = np.ascontiguousarray(mx_off, np.uint64)
        h = np.ascontiguousarray(mx_hash, np.uint64); q = np.ascontiguousarray(pos, np.uint32)
        s = np.ascontiguousarray(strand, np.uint8)
        p = C.c_void_p()
        self._chk(self.L.ntl_sketch_from_host(self.ptr, len(mx_off) - 1, _ptr(mx_off, C.c_uint64), _ptr(h, C.c_uint64),
                                              _ptr(q, C.c_uint32), _ptr(s, C.c_uint8), C.byref(p)))
        return Sketch(self, p)

    def overlap_filter(self, sketch, region_off, region_start, region_end):
        """Valid-region filter + per-sequence duplicate removal of the overlap stage (ntl_overlap_filter) -> new Sketch."""
        ro = np.ascontiguousarray(region_off, np.uint64)
        if len(ro) != sketch.nseq + 1:
            raise ValueError("region_off must have nseq + 1 entries")
        rs = np.ascontiguousarray(region_start, np.uint32); re = np.ascontiguousarray(region_end, np.uint32)
        if len(rs) != int(ro[-1]) or len(re) != len(rs):
            raise ValueError("region arrays must hold region_off[-1] entries")
        if len(rs) == 0:
            rs = np.zeros(1, np.uint32); re = np.zeros(1, np.uint32)
        p = C.c_void_p()
        self._chk(self.L.ntl_overlap_filter(self.ptr, sketch.ptr, _ptr(ro, C.c_uint64), _ptr(rs, C.c_uint32), _ptr(re, C.c_uint32),
                                            C.byref(p)))
        return Sketch(self, p)

    def overlap_cuts(self, sketch, pairs):
        """The cut points of adjacent overlapping contigs (ntl_overlap_cuts, csrc/overlap_cut_kernels.h): `sketch` as overlap_filter
        returns it, `pairs` OVERLAP_PAIR_DT records (or tuples) -- the two sequence numbers, each side's inclusive valid region, the
        two lengths, the signs.  -> OVERLAP_CUT_DT records, one per pair: status (NTL_OVERLAP_CUT: a cut was found), the numbers of
        shared minimizers and of components, the two cuts and the chosen minimizer.  Waits for the device."""
        pr = np.ascontiguousarray(pairs if isinstance(pairs, np.ndarray) else np.array(list(pairs), OVERLAP_PAIR_DT), OVERLAP_PAIR_DT)
        if pr.ndim != 1:
            raise ValueError("pairs must be one-dimensional")
        out = np.zeros(len(pr), OVERLAP_CUT_DT)
        self._chk(self.L.ntl_overlap_cuts(self.ptr, sketch.ptr, pr.ctypes.data if len(pr) else None, len(pr), out.ctypes.data if len(pr) else None))
        return out

    def path_chains(self, n_vertices, edges, links=None, mode=NTL_PATH_STITCH):
        """The graph half of the stitch-paths stage (ntl_path_chains, csrc/path_kernels.h): vertices 2 * contig + (ori == '-'), `edges`
        PATH_EDGE_DT records (or tuples) src, tgt, d, n, flags -- every edge beside its twin (tgt ^ 1, src ^ 1) --, `links` the
        scaffold graph's edges as PATH_LINK_DT (read with mode NTL_PATH_TRANSITIVE only).  -> (chain_off u32[n_chains + 1],
        chain_vertex u32, chain_d i32, counts): the vertices of every emitted chain from head to tail, beside each the d of the edge
        behind it (0 beside the last), and the PATH_COUNTS_DT record.  Waits for the device."""
        ed = np.ascontiguousarray(edges if isinstance(edges, np.ndarray) else np.array(list(edges), PATH_EDGE_DT), PATH_EDGE_DT)
        lk = np.zeros(0, PATH_LINK_DT) if links is None else \
            np.ascontiguousarray(links if isinstance(links, np.ndarray) else np.array(list(links), PATH_LINK_DT), PATH_LINK_DT)
        if ed.ndim != 1 or lk.ndim != 1:
            raise ValueError("edges and links must be one-dimensional")
        n_vertices = int(n_vertices)
        if not 0 <= n_vertices < 1 << 31:
            raise ValueError("n_vertices must be in 0 .. 2^31 - 1")
        off = np.zeros(n_vertices // 2 + 1, np.uint32)
        vertex, d = np.zeros(max(n_vertices, 1), np.uint32), np.zeros(max(n_vertices, 1), np.int32)
        counts = np.zeros(1, PATH_COUNTS_DT)
        self._chk(self.L.ntl_path_chains(self.ptr, n_vertices, ed.ctypes.data if len(ed) else None, len(ed), lk.ctypes.data if len(lk) else None,
                                         len(lk), int(mode), off.ctypes.data, vertex.ctypes.data, d.ctypes.data, counts.ctypes.data))
        n_chains, total = int(counts["n_chains"][0]), int(counts["n_chain_vertices"][0])
        return off[:n_chains + 1].copy(), vertex[:total].copy(), d[:total].copy(), counts[0]

    def gap_select(self, block, ctg_len, large_k, table):
        """The candidates of one block of verbose mappings (ntl_gap_select, csrc/gap_select_kernels.h): `block` as formats.read_verbose
        yields it (.map_off .maps .anchors .hits), ctg_len[n_ctg] of the reader's contig table, `table` = pair_table(keys).  ->
        GAP_CAND_DT records in the order read, combination, direct before reverse complement."""
        mo = np.ascontiguousarray(block.map_off, np.uint32); maps = np.ascontiguousarray(block.maps, MAPPING_DT)
        anc = np.ascontiguousarray(block.anchors, np.uint32); hits = np.ascontiguousarray(block.hits, HIT_DT)
        cl = np.ascontiguousarray(ctg_len, np.uint32)
        keys, vals = np.ascontiguousarray(table[0], np.uint64), np.ascontiguousarray(table[1], np.uint32)
        if len(anc) != len(maps) or len(vals) != len(keys) or len(mo) < 1:
            raise ValueError("one anchors entry per mapping, one value per slot, n_reads + 1 offsets")
        p = C.c_void_p()
        self._chk(self.L.ntl_gap_select(self.ptr, mo.ctypes.data, len(mo) - 1, maps.ctypes.data, anc.ctypes.data, len(maps), hits.ctypes.data, len(hits),
                                        cl.ctypes.data, len(cl), int(large_k), keys.ctypes.data, vals.ctypes.data, len(keys), C.byref(p)))
        try:
            out = np.empty(int(self.L.ntl_gap_cands_count(p)), GAP_CAND_DT)
            self._chk(self.L.ntl_gap_cands_copy(p, out.ctypes.data))
        finally:
            self.L.ntl_gap_cands_destroy(p)
        return out

    def names(self, names, lengths):
        """Device copy of a name table (seqio.Names or a list of str / bytes) with the sequences' lengths."""
        from .seqio import Names
        nm = Names.of(names)
        blob = np.ascontiguousarray(nm.blob)
        off = np.ascontiguousarray(nm.off, np.uint64)
        ln = np.ascontiguousarray(lengths, np.uint32)
        if len(ln) != len(nm):
            raise ValueError("one length per name")
        p = C.c_void_p()
        self._chk(self.L.ntl_names_create(self.ptr, blob.ctypes.data if len(blob) else None, _ptr(off, C.c_uint64),
                                          _ptr(ln, C.c_uint32) if len(ln) else None, len(nm), C.byref(p)))
        return NameTable(self, p)

    def index(self, contig_sketch, ctg_len):
        cl = np.ascontiguousarray(ctg_len, np.uint32)
        p = C.c_void_p()
        self._chk(self.L.ntl_index_build(self.ptr, contig_sketch.ptr, _ptr(cl, C.c_uint32), len(cl), C.byref(p)))
        return Index(self, p)

    def map(self, index, read_sketch, read_len, k, z=1000, x=0.0, sensitive=False, repeat_filter=False):
        rl = np.ascontiguousarray(read_len, np.uint32)
        if len(rl) != read_sketch.nseq:
            raise ValueError("read_len must have one entry per sketched read")
        P = MapParams(int(k), int(z), float(x), int(bool(sensitive)), int(bool(repeat_filter)))
        p = C.c_void_p()
        self._chk(self.L.ntl_map_run(self.ptr, index.ptr, read_sketch.ptr, _ptr(rl, C.c_uint32), C.byref(P),
                                     C.byref(p)))
        return MapResult(self, p)

    def mapres_from_host(self, maps, hit_slots, pafs):
        """A completed MapResult of the caller's records (ntl_mapres_from_host, the map side's sketch_from_arrays): maps (MAPPING_DT)
        whose hit_off index hit_slots (HIT_DT), the hit array as the device keeps it -- regions that ascend with the mapping number,
        unused slots allowed in front of, between and behind them -- and pafs (PAF_DT).  download() gives the dense restatement."""
        m = np.ascontiguousarray(maps, MAPPING_DT); h = np.ascontiguousarray(hit_slots, HIT_DT); q = np.ascontiguousarray(pafs, PAF_DT)
        p = C.c_void_p()
        self._chk(self.L.ntl_mapres_from_host(self.ptr, m.ctypes.data if len(m) else None, len(m), h.ctypes.data if len(h) else None, len(h),
                                              q.ctypes.data if len(q) else None, len(q), C.byref(p)))
        return MapResult(self, p)

    def mapres_liftover(self, result, table, k):
        """`result` lifted through an AGP on the device (ntl_mapres_liftover, csrc/liftover_kernels.h): table = LIFT_ENTRY_DT records (or
        tuples), one per contig number of the result's contig name space -- liftover.lift_table makes it from an AGP.  -> a new,
        completed MapResult in the output name space (no PAF records); `result` is completed, left alone and may be closed."""
        tb = np.ascontiguousarray(table if isinstance(table, np.ndarray) else np.array(list(table), LIFT_ENTRY_DT), LIFT_ENTRY_DT)
        if tb.ndim != 1:
            raise ValueError("table must be one-dimensional")
        p = C.c_void_p()
        self._chk(self.L.ntl_mapres_liftover(self.ptr, result.ptr, tb.ctypes.data if len(tb) else None, len(tb), int(k), C.byref(p)))
        return MapResult(self, p)

    def pair_table(self, tally):
        """The device's copy of what the pair rules need of `tally` (a pairing.PairTally): name rank and length per contig, k and f
        (ntl_pairtab_create).  Serves every context of this GPU (Device.workers); the tally may go on being filled."""
        p = C.c_void_p()
        self._chk(self.L.ntl_pairtab_create(self.ptr, tally._h, C.byref(p)))
        return PairTable(self, p)

    def mapres_pairs(self, result, table, read_len=None):
        """The pair records of `result`, made on the device (ntl_mapres_pairs, csrc/pair_kernels.h): a PAIR_REC_DT array with one record
        per pair PairTally.add_batch would record for the same mappings, in its order -- what PairTally.add_pairs takes.  read_len is
        indexed by the mappings' .read; None: a read's length is the largest read position among the first and last hits of its
        mappings (the checkpoint rule).  No mapping and no hit comes to the host.  `result` is completed and left alone; it may belong
        to another context of this GPU than `table`."""
        dev = result.dev
        rl = None if read_len is None else np.ascontiguousarray(read_len, np.uint32)
        held = None if rl is None else rl if len(rl) else np.zeros(1, np.uint32)  # (an empty array is still "given": a pointer, n_reads = 0)
        p = C.c_void_p()
        dev._chk(dev.L.ntl_mapres_pairs(result.ptr, table.ptr, None if held is None else _ptr(held, C.c_uint32), 0 if rl is None else len(rl),
                                        C.byref(p)))
        try:
            out = np.empty(int(dev.L.ntl_pairs_count(p)), PAIR_REC_DT)
            dev._chk(dev.L.ntl_pairs_download(p, out.ctypes.data if len(out) else None))
        finally:
            dev.L.ntl_pairs_destroy(p)
        return out

    def map_grouped(self, contig_sketch, ctg_len, ctg_group_off, read_sketch, read_len, read_group_off, k, z=1000, x=0.0, sensitive=False,
                    repeat_filter=False):
        """Device.index + Device.map once per group, in one device pass (ntl_map_run_grouped): group g = the contigs
        [ctg_group_off[g], ctg_group_off[g+1]) and the reads [read_group_off[g], read_group_off[g+1]); a hash that occurs twice among
        one group's contigs is dropped for that group only, a read is looked up in its own group only.  Contig and read numbers of the
        result are those of the two sketches.  Both sketches and every array may go once this returns."""
        cl = np.ascontiguousarray(ctg_len, np.uint32); rl = np.ascontiguousarray(read_len, np.uint32)
        co = np.ascontiguousarray(ctg_group_off, np.uint32); ro = np.ascontiguousarray(read_group_off, np.uint32)
        if len(cl) != contig_sketch.nseq or len(rl) != read_sketch.nseq:
            raise ValueError("ctg_len / read_len must have one entry per sketched sequence")
        if len(co) != len(ro) or len(co) < 1:
            raise ValueError("the group offsets must have n_groups + 1 entries each")
        P = MapParams(int(k), int(z), float(x), int(bool(sensitive)), int(bool(repeat_filter)))
        p = C.c_void_p()
        self._chk(self.L.ntl_map_run_grouped(self.ptr, contig_sketch.ptr, _ptr(cl, C.c_uint32), _ptr(co, C.c_uint32), read_sketch.ptr,
                                             _ptr(rl, C.c_uint32), _ptr(ro, C.c_uint32), len(co) - 1, C.byref(P), C.byref(p)))
        return MapResult(self, p)


def pair_key(src_ctg, src_minus, tgt_ctg, tgt_minus):
    """the 64-bit key of a path pair in ntl_gap_select's table: source node << 32 | target node, node = contig << 1 | minus"""
    return ((int(src_ctg) << 1 | int(bool(src_minus))) << 32) | (int(tgt_ctg) << 1 | int(bool(tgt_minus)))


def pair_table(keys, n_slots=None, lib_path=None):
    """(slot_keys u64, slot_vals u32) of ntl_gap_pair_table: keys[i] is pair i; by default the smallest power of two of slots that
    leaves the table at most half full."""
    keys = np.ascontiguousarray(keys, np.uint64)
    if n_slots is None:
        n_slots = 2
        while n_slots < 2 * len(keys):
            n_slots *= 2
    sk, sv = np.empty(n_slots, np.uint64), np.empty(n_slots, np.uint32)
    if load(lib_path).ntl_gap_pair_table(keys.ctypes.data, len(keys), sk.ctypes.data, sv.ctypes.data, n_slots) != 0:
        raise ValueError("ntl_gap_pair_table: distinct keys and a power of two of at least twice as many slots are needed")
    return sk, sv
