"""ctypes binding of libherro_amd.so (include/herro_amd.h).  Fails loudly if the HIP library is
missing or no GPU is present — there is no CPU fallback in this package."""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HERRO_LIB: another build of the same library (e.g. the HERRO_PROF_BUILD one of tools/prof.sh), for A/B runs on one GPU box
LIB_PATH = os.environ.get("HERRO_LIB") or os.path.join(_HERE, "libherro_amd.so")
_LIB = None
# GEMM precision used by bench.py / smoke / the end-to-end tests (herro_set_precision): 1 = bf16 hi/lo x3,
# 4 = f16 (conv / FC / attention single, encoder GEMMs activation hi + lo), see csrc/model_h.hip; 6 = 4 with the activation remainder as e4m3 on the
# K = 128 MX MFMA (same contract, measured no faster on an MI355X: not the default)
DEFAULT_PRECISION = 4

EXPORTS = [
    "herro_version", "herro_create", "herro_destroy", "herro_last_error", "herro_set_stream", "herro_synchronize",
    "herro_encode_2bit", "herro_decode_2bit", "herro_set_reads", "herro_set_reads_packed", "herro_share_reads", "herro_load_model",
    "herro_set_precision", "herro_precision", "herro_clock_probe", "herro_calibration_error", "herro_debug_force_precision", "herro_model_describe", "herro_job_create", "herro_job_free", "herro_job_n_windows", "herro_job_skipped", "herro_job_featurize",
    "herro_job_infer", "herro_job_consensus", "herro_job_consensus_fetch", "herro_job_window_info", "herro_job_window_copy", "herro_job_window_logits",
    "herro_job_consensus_fasta", "herro_job_fasta", "herro_model_forward", "herro_timing_enable", "herro_timing_reset",
    "herro_timing_get", "herro_job_stats", "herro_debug_extract_windows",
    "herro_paf_parse", "herro_oec_read", "herro_paf_n_targets", "herro_paf_target_ids", "herro_paf_aln_off",
    "herro_paf_alignments", "herro_paf_free", "herro_name_index_create", "herro_name_index_free", "herro_paf_parse_indexed",
    "herro_oec_read_indexed", "herro_paf_parse_view", "herro_debug_host_ctx", "herro_debug_job_array", "herro_debug_tile_plan", "herro_debug_tile_plan_sib", "herro_debug_launch_plan",
    "herro_debug_set_featurize_planes", "herro_debug_set_conv_fc", "herro_debug_set_front_cu", "herro_debug_front_last", "herro_debug_front_end_plan", "herro_debug_set_host_build", "herro_debug_job_dev_built", "herro_debug_job_rf", "herro_debug_job_cwd", "herro_debug_job_set_base_logits", "herro_debug_job_rf_fused", "herro_debug_job_rf_left", "herro_debug_e4m3", "herro_debug_model_pack", "herro_debug_sib_fault", "herro_debug_sib_retries", "herro_debug_base_row_votes", "herro_debug_vote5",
    "herro_pool_create", "herro_pool_destroy", "herro_pool_last_error", "herro_pool_size", "herro_pool_ctx", "herro_pool_set_reads", "herro_pool_load_model",
    "herro_pool_correct", "herro_pool_result", "herro_pool_groups_taken", "herro_pool_skipped", "herro_debug_pool_fake", "herro_job_create_status", "herro_host_register", "herro_host_unregister", "herro_debug_zero_copy_jobs",
    "herro_fastx_read", "herro_reads_count", "herro_reads_seq", "herro_reads_qual", "herro_reads_off", "herro_reads_ids",
    "herro_reads_descs", "herro_reads_free", "herro_write_window_features", "herro_job_write_features",
    "herro_paf_parse_coords", "herro_align_overlaps", "herro_aligned_alignments", "herro_aligned_scores", "herro_aligned_failed",
    "herro_aligned_free",
    "herro_align_overlaps_dev", "herro_aligned_dev_from_ops", "herro_aligned_dev_mirror", "herro_aligned_dev_n", "herro_aligned_dev_alignments", "herro_aligned_dev_scores",
    "herro_aligned_dev_n_ops", "herro_aligned_dev_failed", "herro_aligned_dev_cigar", "herro_aligned_dev_free", "herro_job_create_aligned",
    "herro_find_overlaps", "herro_overlaps_n", "herro_overlaps_n_targets", "herro_overlaps_target_ids", "herro_overlaps_aln_off",
    "herro_overlaps_alignments", "herro_overlaps_scores", "herro_overlaps_free", "herro_debug_sketch",
    "herro_extend_overlaps", "herro_extended_n", "herro_extended_alignments", "herro_extended_ext", "herro_extended_scores", "herro_extended_free",
    "herro_find_overlap_pairs", "herro_pairs_from_table", "herro_pairs_align", "herro_job_create_paired", "herro_pairs_n", "herro_pairs_primaries",
    "herro_pairs_chain_scores", "herro_pairs_ext", "herro_pairs_ext_scores", "herro_pairs_n_targets", "herro_pairs_target_ids", "herro_pairs_aln_off",
    "herro_pairs_rec_of_row", "herro_pairs_free",
    "herro_find_overlaps_core", "herro_find_overlap_pairs_core", "herro_pairs_from_table_core", "herro_pairs_n_rows",
    "herro_overlaps_occ_cut", "herro_pairs_occ_cut", "herro_debug_occ_census",
    "herro_aligned_dev_paf", "herro_pairs_paf", "herro_paf_text_data", "herro_paf_text_len", "herro_paf_text_lines", "herro_paf_text_free",
    "herro_pairs_write_alns",
    "herro_set_seed_rescue", "herro_overlaps_rescued", "herro_pairs_rescued", "herro_debug_seed_rescue",
    "herro_set_chain_params", "herro_debug_chain",
    "herro_find_adapters", "herro_adapter_hits_n", "herro_adapter_hits_data", "herro_adapter_hits_off", "herro_adapter_hits_free", "herro_debug_set_adapter_cap",
    "herro_trim_plan", "herro_trim_n_pieces", "herro_trim_pieces", "herro_trim_piece_off", "herro_trim_stats", "herro_trim_free",
    "herro_reads_create", "herro_reads_cut", "herro_reads_cut_names",
    "herro_store_cut", "herro_debug_store_copy", "herro_debug_scan_u32", "herro_debug_radix_sort", "herro_debug_offsets64",
    "herro_cluster_graph", "herro_pairs_cluster", "herro_clusters_n_parts", "herro_clusters_n_reads", "herro_clusters_part", "herro_clusters_rank",
    "herro_clusters_comp", "herro_clusters_level", "herro_clusters_stats", "herro_clusters_part_stats", "herro_clusters_mask", "herro_clusters_free",
    "herro_job_fasta_dev", "herro_fasta_text_data", "herro_fasta_text_len", "herro_fasta_text_target_end", "herro_fasta_text_stats", "herro_fasta_text_free",
    "herro_debug_set_fasta_chunk", "herro_chop_plan",
    "herro_set_index_params", "herro_overlaps_index_blocks", "herro_pairs_index_blocks", "herro_index_plan",
]


class HerroError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"herro_amd error {code}: {msg}")
        self.code = code


class Alignment(C.Structure):  # herro_alignment
    _fields_ = [(n, C.c_uint32) for n in
                ("qid", "qlen", "qstart", "qend", "strand", "tid", "tlen", "tstart", "tend", "cigar_len")] + \
               [("cigar", C.c_void_p)]


ALN_DTYPE = np.dtype([("f", np.uint32, 10), ("p", np.uint64)], align=True)   # herro_alignment as numpy sees it: f = the ten u32 fields, p = cigar


def _aln_array(rows: np.ndarray, ncols: int = 9):
    """rows u32 [n, >= ncols] -> (an Alignment array of max(n, 1) with those columns filled in and the rest 0, its ALN_DTYPE view)"""
    n = len(rows)
    arr = (Alignment * max(n, 1))()
    view = np.frombuffer(arr, dtype=ALN_DTYPE, count=max(n, 1))   # vectorised fill through a numpy view of the ctypes array
    if n:
        view["f"][:n, :ncols] = rows[:, :ncols]
    return arr, view


def _aln_rows(ptr, n: int, with_cigar_ptr: bool = False):
    """the n herro_alignment at ptr -> rows u32 [n, 10] (a copy; with_cigar_ptr: and their cigar pointers u64 [n])"""
    rows, cig = np.zeros((n, 10), np.uint32), np.zeros(n, np.uint64)
    if n:
        view = np.frombuffer((Alignment * n).from_address(ptr), dtype=ALN_DTYPE, count=n)
        rows[:], cig[:] = view["f"], view["p"]
    return (rows, cig) if with_cigar_ptr else rows


def _job_or_raise(ctx: "Context", h, n_targets: int) -> "Job":
    """herro_job_create*'s handle as a Job; NULL: HerroError with the code its message ends on"""
    if not h:
        msg = ctx._l.herro_last_error(ctx.h).decode(errors="replace")
        code = int(msg.rsplit("[code ", 1)[1].rstrip("]")) if "[code " in msg else -1
        raise HerroError(code, msg)
    return Job(ctx, h, n_targets)


PAIRS_NO_EXTEND = 1   # HERRO_PAIRS_NO_EXTEND
ALNS_OEC = 1          # HERRO_ALNS_OEC


class OverlapParams(C.Structure):  # herro_overlap_params (0 = the field's default)
    _fields_ = [(n, C.c_uint32) for n in ("k", "w", "max_occ", "bandwidth", "max_gap", "min_score", "min_anchors", "occ_frac_ppm")]


class SeedRescueParams(C.Structure):  # herro_seed_rescue_params (occ_dist 0 = off, rescue_max_occ 0 = 4095)
    _fields_ = [("occ_dist", C.c_uint32), ("rescue_max_occ", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ChainParams(C.Structure):  # herro_chain_params (lookback 0 = 64)
    _fields_ = [("lookback", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class IndexParams(C.Structure):  # herro_index_params (max_kmers 0 = off, occ_ranges 0 = chosen by the library)
    _fields_ = [("max_kmers", C.c_uint64), ("occ_ranges", C.c_uint32), ("reserved", C.c_uint32)]


class ExtendParams(C.Structure):  # herro_extend_params (0 = the field's default)
    _fields_ = [("zdrop", C.c_uint32), ("max_ext", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ClusterParams(C.Structure):  # herro_cluster_params
    _fields_ = [("n_parts", C.c_uint32), ("min_span", C.c_uint32), ("reserved", C.c_uint32 * 2)]


ADAPTERS_FORWARD_ONLY = 1    # HERRO_ADAPTERS_FORWARD_ONLY
TRIM_DISCARD_CHIMERAS = 1    # HERRO_TRIM_DISCARD_CHIMERAS
ADAPTER_HIT_DTYPE = np.dtype([("rid", "<u4"), ("start", "<u4"), ("end", "<u4"), ("adapter", "<u2"), ("strand", "u1"), ("errors", "u1")])   # herro_adapter_hit
PIECE_DTYPE = np.dtype([("rid", "<u4"), ("start", "<u4"), ("end", "<u4")])   # herro_piece


class AdapterParams(C.Structure):  # herro_adapter_params (0 = the field's default)
    _fields_ = [("max_err_pm", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ChopParams(C.Structure):  # herro_chop_params (0 = off)
    _fields_ = [(n, C.c_uint32) for n in ("chop_len", "min_length", "line_width", "flags")] + [("reserved", C.c_uint32 * 4)]


# scripts/postprocess_corrected.sh of the reference's workflow: `seqkit sliding -s 30000 -W 30000 -g`, then `seqkit seq -m 10000`
POSTPROCESS = dict(chop_len=30000, min_length=10000)


class TrimParams(C.Structure):  # herro_trim_params (0 = the field's default)
    _fields_ = [(n, C.c_uint32) for n in ("end_window", "end_max_err_pm", "mid_max_err_pm", "min_length", "flags")] + [("reserved", C.c_uint32 * 3)]


class WindowInfo(C.Structure):  # herro_window_info
    _fields_ = [(n, C.c_uint32) for n in
                ("rid", "wid", "n_total_wins", "length", "n_alns", "n_overlaps", "n_supported", "win_len")]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built — run __graft_entry__.build(); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        L.herro_version.restype = C.c_char_p
        L.herro_create.restype = vp
        L.herro_create.argtypes = [i32]
        L.herro_destroy.argtypes = [vp]
        L.herro_last_error.restype = C.c_char_p
        L.herro_last_error.argtypes = [vp]
        L.herro_set_stream.argtypes = [vp, vp]
        L.herro_synchronize.argtypes = [vp]
        L.herro_encode_2bit.restype = C.c_int64
        L.herro_encode_2bit.argtypes = [vp, u64, vp]
        L.herro_decode_2bit.argtypes = [vp, u64, u64, u64, i32, vp]
        L.herro_set_reads.argtypes = [vp, u32, vp, vp, vp, vp]
        L.herro_set_reads_packed.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.herro_share_reads.argtypes = [vp, vp]
        L.herro_pool_create.restype = vp
        L.herro_pool_create.argtypes = [vp, u32]
        L.herro_pool_destroy.argtypes = [vp]
        L.herro_pool_last_error.restype = C.c_char_p
        L.herro_pool_last_error.argtypes = [vp]
        L.herro_pool_size.restype = u32
        L.herro_pool_size.argtypes = [vp]
        L.herro_pool_ctx.restype = vp
        L.herro_pool_ctx.argtypes = [vp, u32]
        L.herro_pool_set_reads.argtypes = [vp, u32, vp, vp, vp, vp]
        L.herro_pool_load_model.argtypes = [vp, C.c_char_p]
        L.herro_pool_correct.restype = C.c_int64
        L.herro_pool_correct.argtypes = [vp, u32, vp, vp, vp, u32, u32, i32, u32, vp, vp]
        L.herro_pool_result.restype = vp
        L.herro_pool_result.argtypes = [vp, vp]
        L.herro_pool_groups_taken.restype = u32
        L.herro_pool_groups_taken.argtypes = [vp, u32]
        L.herro_pool_skipped.argtypes = [vp, vp, vp]
        L.herro_debug_pool_fake.restype = vp
        L.herro_debug_pool_fake.argtypes = [u32, vp]
        L.herro_job_create_status.argtypes = [vp]
        L.herro_host_register.argtypes = [vp, vp, u64]
        L.herro_host_unregister.argtypes = [vp, vp]
        L.herro_debug_zero_copy_jobs.restype = u64
        L.herro_debug_zero_copy_jobs.argtypes = []
        L.herro_load_model.argtypes = [vp, C.c_char_p]
        L.herro_set_precision.argtypes = [vp, i32]
        try:   # (an older build of the library selected by HERRO_LIB for a same-box A/B lacks the round-6 entries)
            L.herro_precision.argtypes = [vp]
            L.herro_calibration_error.restype = C.c_float
            L.herro_calibration_error.argtypes = [vp, i32]
            L.herro_debug_force_precision.argtypes = [vp, i32]
            L.herro_clock_probe.argtypes = [vp, vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        L.herro_job_create.restype = vp
        L.herro_job_create.argtypes = [vp, u32, vp, vp, vp, u32]
        L.herro_job_free.argtypes = [vp]
        L.herro_job_n_windows.restype = u32
        L.herro_job_n_windows.argtypes = [vp]
        L.herro_job_skipped.argtypes = [vp, vp, vp]
        L.herro_job_featurize.argtypes = [vp]
        L.herro_job_infer.argtypes = [vp, u32, i32]
        L.herro_job_consensus.argtypes = [vp]
        L.herro_job_consensus_fetch.argtypes = [vp, vp]
        L.herro_job_window_info.argtypes = [vp, u32, vp]
        L.herro_job_window_copy.argtypes = [vp, u32, i32, vp, vp, vp, vp, vp]
        L.herro_job_window_logits.argtypes = [vp, u32, vp, vp]
        L.herro_job_consensus_fasta.restype = C.c_int64
        L.herro_job_consensus_fasta.argtypes = [vp, u32, C.c_char_p, C.c_char_p, vp, u64]
        L.herro_model_describe.restype = C.c_int64
        L.herro_model_describe.argtypes = [vp, vp, u64]
        L.herro_job_fasta.restype = C.c_int64
        L.herro_job_fasta.argtypes = [vp, vp, vp, vp, u64, vp]
        L.herro_model_forward.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, vp]
        L.herro_timing_enable.argtypes = [vp, i32]
        L.herro_timing_reset.argtypes = [vp]
        L.herro_timing_get.argtypes = [vp, vp, u64, vp, vp, vp]
        L.herro_job_stats.argtypes = [vp, vp]
        L.herro_debug_extract_windows.restype = C.c_int64
        L.herro_debug_extract_windows.argtypes = [vp, u32, u32, vp, u64, vp, u64]
        L.herro_paf_parse.restype = vp
        L.herro_paf_parse.argtypes = [C.c_char_p, u64, u32, C.c_char_p, vp, vp, i32, vp, u64]
        L.herro_oec_read.restype = vp
        L.herro_oec_read.argtypes = [C.c_char_p, u32, C.c_char_p, vp, vp, i32, vp, u64]
        L.herro_paf_n_targets.restype = u32
        L.herro_paf_n_targets.argtypes = [vp]
        for f in (L.herro_paf_target_ids, L.herro_paf_aln_off, L.herro_paf_alignments):
            f.restype = vp
            f.argtypes = [vp]
        L.herro_paf_free.restype = None
        L.herro_paf_free.argtypes = [vp]
        L.herro_name_index_create.restype = vp
        L.herro_name_index_create.argtypes = [u32, C.c_char_p, vp]
        L.herro_name_index_free.restype = None
        L.herro_name_index_free.argtypes = [vp]
        L.herro_paf_parse_indexed.restype = vp
        L.herro_paf_parse_indexed.argtypes = [C.c_char_p, u64, vp, vp, i32, vp, u64]
        L.herro_oec_read_indexed.restype = vp
        L.herro_oec_read_indexed.argtypes = [C.c_char_p, vp, vp, i32, vp, u64]
        L.herro_paf_parse_view.restype = vp
        L.herro_paf_parse_view.argtypes = [C.c_char_p, u64, vp, vp, i32, vp, u64]
        L.herro_paf_parse_coords.restype = vp
        L.herro_paf_parse_coords.argtypes = [C.c_char_p, u64, vp, vp, i32, vp, u64]
        L.herro_align_overlaps.argtypes = [vp, u32, vp, vp]
        L.herro_aligned_alignments.restype = vp
        L.herro_aligned_alignments.argtypes = [vp]
        L.herro_aligned_scores.restype = vp
        L.herro_aligned_scores.argtypes = [vp]
        L.herro_aligned_failed.restype = u32
        L.herro_aligned_failed.argtypes = [vp]
        L.herro_aligned_free.restype = None
        L.herro_aligned_free.argtypes = [vp]
        L.herro_align_overlaps_dev.argtypes = [vp, u32, vp, vp]
        L.herro_aligned_dev_from_ops.argtypes = [vp, u32, vp, vp, vp, vp]
        L.herro_aligned_dev_mirror.argtypes = [vp, vp, vp]
        for f in (L.herro_aligned_dev_n, L.herro_aligned_dev_failed):
            f.restype = u32
            f.argtypes = [vp]
        for f in (L.herro_aligned_dev_alignments, L.herro_aligned_dev_scores, L.herro_aligned_dev_n_ops):
            f.restype = vp
            f.argtypes = [vp]
        L.herro_aligned_dev_cigar.restype = C.c_int64
        L.herro_aligned_dev_cigar.argtypes = [vp, u32, vp, u64]
        L.herro_aligned_dev_free.restype = None
        L.herro_aligned_dev_free.argtypes = [vp]
        L.herro_job_create_aligned.restype = vp
        L.herro_job_create_aligned.argtypes = [vp, u32, vp, vp, vp, vp, u32]
        L.herro_find_overlaps.argtypes = [vp, vp, vp]
        for f in (L.herro_overlaps_n, L.herro_overlaps_n_targets):
            f.restype = u32
            f.argtypes = [vp]
        for f in (L.herro_overlaps_target_ids, L.herro_overlaps_aln_off, L.herro_overlaps_alignments, L.herro_overlaps_scores):
            f.restype = vp
            f.argtypes = [vp]
        L.herro_overlaps_free.restype = None
        L.herro_overlaps_free.argtypes = [vp]
        L.herro_extend_overlaps.argtypes = [vp, u32, vp, vp, vp]
        L.herro_extended_n.restype = u32
        L.herro_extended_n.argtypes = [vp]
        for f in (L.herro_extended_alignments, L.herro_extended_ext, L.herro_extended_scores):
            f.restype = vp
            f.argtypes = [vp]
        L.herro_extended_free.restype = None
        L.herro_extended_free.argtypes = [vp]
        L.herro_find_overlap_pairs.argtypes = [vp, vp, vp, u32, vp]
        L.herro_pairs_from_table.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp, vp]
        L.herro_pairs_align.argtypes = [vp, vp, vp]
        L.herro_job_create_paired.restype = vp
        L.herro_job_create_paired.argtypes = [vp, vp, vp, u32]
        for f in (L.herro_pairs_n, L.herro_pairs_n_targets):
            f.restype = u32
            f.argtypes = [vp]
        for f in (L.herro_pairs_primaries, L.herro_pairs_chain_scores, L.herro_pairs_ext, L.herro_pairs_ext_scores, L.herro_pairs_target_ids,
                  L.herro_pairs_aln_off, L.herro_pairs_rec_of_row):
            f.restype = vp
            f.argtypes = [vp]
        L.herro_pairs_free.restype = None
        L.herro_pairs_free.argtypes = [vp]
        try:   # (an older build selected by HERRO_LIB lacks the core-mask entries: its unmasked calls still run)
            L.herro_find_overlaps_core.argtypes = [vp, vp, vp, vp]
            L.herro_find_overlap_pairs_core.argtypes = [vp, vp, vp, u32, vp, vp]
            L.herro_pairs_from_table_core.argtypes = [vp, u32, vp, vp, u32, vp, vp, u64, vp, vp]
            L.herro_pairs_n_rows.restype = u64
            L.herro_pairs_n_rows.argtypes = [vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the fraction cut: its calls with occ_frac_ppm left out still run)
            for f in (L.herro_overlaps_occ_cut, L.herro_pairs_occ_cut):
                f.restype = u32
                f.argtypes = [vp]
            L.herro_debug_occ_census.argtypes = [vp, vp, vp, vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the rescue: every call that leaves it off still runs)
            L.herro_set_seed_rescue.argtypes = [vp, vp]
            for f in (L.herro_overlaps_rescued, L.herro_pairs_rescued):
                f.restype = u32
                f.argtypes = [vp]
            L.herro_debug_seed_rescue.restype = C.c_int64
            L.herro_debug_seed_rescue.argtypes = [vp, vp, vp, vp, u64]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the chain look-back: every call that leaves it at 64 still runs)
            L.herro_set_chain_params.argtypes = [vp, vp]
            L.herro_debug_chain.argtypes = [vp, u64, vp, vp, vp, vp, vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the index in parts: every call that leaves it off still runs)
            L.herro_set_index_params.argtypes = [vp, vp]
            for f in (L.herro_overlaps_index_blocks, L.herro_pairs_index_blocks):
                f.restype = u32
                f.argtypes = [vp]
            L.herro_index_plan.restype = C.c_int64
            L.herro_index_plan.argtypes = [vp, u64, vp, u32, u32, u64, vp, u64]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the PAF writer: everything else still runs)
            L.herro_aligned_dev_paf.argtypes = [vp, vp, u64, vp, C.c_char_p, vp, vp]
            L.herro_pairs_paf.argtypes = [vp, vp, vp, C.c_char_p, vp, vp]
            L.herro_paf_text_data.restype = vp
            L.herro_paf_text_data.argtypes = [vp]
            for f in (L.herro_paf_text_len, L.herro_paf_text_lines):
                f.restype = u64
                f.argtypes = [vp]
            L.herro_paf_text_free.restype = None
            L.herro_paf_text_free.argtypes = [vp]
            L.herro_pairs_write_alns.argtypes = [vp, vp, vp, C.c_char_p, vp, C.c_char_p, u32, vp, vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the adapter step: everything else still runs)
            L.herro_find_adapters.argtypes = [vp, u32, C.c_char_p, vp, vp, vp]
            L.herro_adapter_hits_n.restype = u64
            L.herro_adapter_hits_n.argtypes = [vp]
            for f in (L.herro_adapter_hits_data, L.herro_adapter_hits_off, L.herro_trim_pieces, L.herro_trim_piece_off):
                f.restype = vp
                f.argtypes = [vp]
            L.herro_adapter_hits_free.restype = None
            L.herro_adapter_hits_free.argtypes = [vp]
            L.herro_debug_set_adapter_cap.argtypes = [vp, u64]
            L.herro_trim_plan.argtypes = [u32, vp, u32, vp, vp, vp, vp, vp, vp, u64]
            L.herro_trim_n_pieces.restype = u64
            L.herro_trim_n_pieces.argtypes = [vp]
            L.herro_trim_stats.argtypes = [vp, vp]
            L.herro_trim_free.restype = None
            L.herro_trim_free.argtypes = [vp]
            L.herro_reads_create.restype = vp
            L.herro_reads_create.argtypes = [u32, vp, vp, vp, vp, vp, vp, u64]
            L.herro_reads_cut.restype = vp
            L.herro_reads_cut.argtypes = [vp, u64, vp, vp, u64]
            L.herro_reads_cut_names.restype = vp
            L.herro_reads_cut_names.argtypes = [u32, vp, vp, vp, u64, vp, vp, u64]
            L.herro_store_cut.argtypes = [vp, u64, vp, vp]
            L.herro_debug_store_copy.restype = C.c_int64
            L.herro_debug_store_copy.argtypes = [vp, C.c_int, vp, u64]
            L.herro_debug_scan_u32.argtypes = [vp, vp, u64, vp, vp]
            L.herro_debug_radix_sort.argtypes = [vp, vp, vp, u64, vp, u32, vp]
            L.herro_debug_offsets64.argtypes = [vp, vp, u64, vp, vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the clusters: everything else still runs)
            L.herro_cluster_graph.argtypes = [vp, u64, vp, u64, vp, vp, vp, vp, vp]
            L.herro_pairs_cluster.argtypes = [vp, vp, vp, vp, vp]
            L.herro_clusters_n_parts.restype = u32
            L.herro_clusters_n_parts.argtypes = [vp]
            L.herro_clusters_n_reads.restype = u64
            L.herro_clusters_n_reads.argtypes = [vp]
            for f in (L.herro_clusters_part, L.herro_clusters_rank, L.herro_clusters_comp, L.herro_clusters_level):
                f.restype = vp
                f.argtypes = [vp]
            L.herro_clusters_stats.argtypes = [vp, vp]
            L.herro_clusters_part_stats.argtypes = [vp, u32, vp]
            L.herro_clusters_mask.argtypes = [vp, u32, vp]
            L.herro_clusters_free.restype = None
            L.herro_clusters_free.argtypes = [vp]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        try:   # (an older build selected by HERRO_LIB lacks the device FASTA: everything else still runs)
            L.herro_job_fasta_dev.argtypes = [vp, vp, vp, vp, vp]
            L.herro_fasta_text_data.restype = vp
            L.herro_fasta_text_data.argtypes = [vp]
            L.herro_fasta_text_len.restype = u64
            L.herro_fasta_text_len.argtypes = [vp]
            L.herro_fasta_text_target_end.restype = vp
            L.herro_fasta_text_target_end.argtypes = [vp]
            L.herro_fasta_text_stats.argtypes = [vp, vp]
            L.herro_fasta_text_free.restype = None
            L.herro_fasta_text_free.argtypes = [vp]
            L.herro_debug_set_fasta_chunk.argtypes = [vp, u64]
            L.herro_chop_plan.argtypes = [u64, vp, vp, vp, vp, u64]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        L.herro_debug_sketch.restype = C.c_int64
        L.herro_debug_sketch.argtypes = [vp, vp, vp, vp, vp, vp, u64]
        L.herro_debug_host_ctx.restype = vp
        L.herro_debug_host_ctx.argtypes = [u32, vp, vp]
        L.herro_debug_job_array.restype = C.c_int64
        L.herro_debug_job_array.argtypes = [vp, i32, vp, vp]
        L.herro_debug_set_featurize_planes.argtypes = [vp, i32]
        L.herro_debug_set_host_build.argtypes = [vp, i32]
        try:   # (an older build selected by HERRO_LIB has the two-kernel front end only)
            L.herro_debug_set_conv_fc.argtypes = [vp, i32]
        except AttributeError:
            if not os.environ.get("HERRO_LIB"):
                raise
        L.herro_debug_set_front_cu.argtypes = [vp, u32]
        L.herro_debug_front_last.argtypes = [vp, vp]
        L.herro_debug_front_end_plan.argtypes = [u32, u32, u32, i32, vp]
        L.herro_debug_job_dev_built.argtypes = [vp]
        L.herro_debug_base_row_votes.argtypes = [vp, vp, vp, u32, vp, vp]
        L.herro_debug_vote5.restype = u32
        L.herro_debug_vote5.argtypes = [vp, u32]
        L.herro_debug_job_rf_fused.argtypes = [vp]
        L.herro_debug_job_rf_left.argtypes = [vp]
        L.herro_debug_sib_fault.argtypes = [vp]
        L.herro_debug_e4m3.argtypes = [C.c_float]
        L.herro_debug_e4m3.restype = C.c_uint32
        L.herro_debug_model_pack.restype = C.c_int64
        L.herro_debug_model_pack.argtypes = [C.c_char_p, C.c_char_p, u32, u32, i32, vp, u64, vp]
        L.herro_debug_sib_retries.argtypes = [vp]
        L.herro_debug_job_rf.restype = C.c_int64
        L.herro_debug_job_rf.argtypes = [vp, u32, vp, u64]
        L.herro_debug_job_cwd.restype = C.c_int64
        L.herro_debug_job_cwd.argtypes = [vp, u32, vp, u64]
        L.herro_debug_job_set_base_logits.argtypes = [vp, vp, u64]
        L.herro_debug_tile_plan.restype = C.c_int64
        L.herro_debug_tile_plan.argtypes = [vp, u32, i32, u32, vp, vp, vp]
        L.herro_debug_tile_plan_sib.restype = i32
        L.herro_debug_tile_plan_sib.argtypes = [vp, u32, i32, u32, vp, vp, vp, vp]
        L.herro_debug_launch_plan.restype = C.c_int64
        L.herro_debug_launch_plan.argtypes = [vp, vp, u32, vp, u32, u32, i32, i32, u32, i32, u32, vp, vp, vp]
        _LIB = L
    return _LIB


def encode_2bit(seq: bytes) -> np.ndarray:
    """haec_io.rs:121-136 (host utility)."""
    words = np.zeros((len(seq) + 31) // 32 + 1, np.uint64)
    buf = np.frombuffer(seq, np.uint8)
    n = lib().herro_encode_2bit(buf.ctypes.data if len(seq) else None, len(seq), words.ctypes.data)
    if n < 0:
        raise HerroError(int(n), "byte >= 128 in sequence")
    return words[:n].copy()


def decode_2bit(words: np.ndarray, length: int, start: int, end: int, rc: bool) -> bytes:
    """haec_io.rs:138-173 (host utility)."""
    words = np.ascontiguousarray(words, np.uint64)
    out = np.zeros(max(end - start, 0), np.uint8)
    r = lib().herro_decode_2bit(words.ctypes.data, length, start, end, int(rc), out.ctypes.data)
    if r:
        raise HerroError(r, "Out of bounds for 2-bit sequence decoding.")
    return out.tobytes()


def debug_extract_windows(row, cigar: bytes, n_windows: int, window_size: int) -> np.ndarray:
    """Product windowing for one alignment (host only).  Rows: window,tstart,qstart,qend,op_lo,op_hi,so,eo."""
    a = Alignment()
    (a.qid, a.qlen, a.qstart, a.qend, a.strand, a.tid, a.tlen, a.tstart, a.tend) = (int(x) for x in row)
    buf = np.frombuffer(cigar + b"\0", np.uint8).copy()
    a.cigar_len, a.cigar = len(cigar), buf.ctypes.data
    out = np.zeros((65536, 8), np.uint64)
    err = C.create_string_buffer(512)
    n = lib().herro_debug_extract_windows(C.byref(a), n_windows, window_size, out.ctypes.data, len(out), err, 512)
    if n < 0:
        raise HerroError(int(n), err.value.decode())
    return out[:n].astype(np.int64)


def debug_tile_plan(counts, packed: bool = True, qmode: int = 0, n_cu: int = 256, bounds: bool = False):
    """(tiles, order) of one fused launch over windows of `counts` informative rows (host only, herro_debug_tile_plan).
    qmode 1 / 2: the plans with 32-token tiles (short last round / every small window) -> (tiles of 64, tiles of 32, order);
    bounds: append the first token of every tile (+ end)."""
    c = np.ascontiguousarray(counts, np.uint32)
    order = np.zeros(max(len(c), 1), np.uint32)
    n_half = C.c_uint32(0)
    tok = np.zeros(len(c) + 2, np.uint32)
    n = lib().herro_debug_tile_plan(c.ctypes.data, len(c), int(packed) | (qmode << 1), n_cu, order.ctypes.data, C.byref(n_half), tok.ctypes.data)
    if n < 0:
        raise HerroError(int(n), "herro_debug_tile_plan")
    out = (int(n), int(n_half.value), order[:len(c)]) if qmode else (int(n), order[:len(c)])
    return out + (tok[:int(n) + int(n_half.value) + 1],) if bounds else out


def debug_tile_plan_sib(counts, packed: bool = True, qmode: int = 1, n_cu: int = 256):
    """Token-tile plan with windows above 64 rows admitted (herro_debug_tile_plan_sib): (n_sibling, n64, n32, order, tile bounds, grp)."""
    c = np.ascontiguousarray(counts, np.uint32)
    order = np.zeros(max(len(c), 1), np.uint32)
    cap = int(((c.astype(np.int64) + 63) // 64).sum()) + 2
    n_tiles = np.zeros(3, np.uint32)
    tok = np.zeros(cap, np.uint32)
    grp = np.zeros(cap, np.uint32)
    rc = lib().herro_debug_tile_plan_sib(c.ctypes.data, len(c), int(packed) | (qmode << 1), n_cu, order.ctypes.data, n_tiles.ctypes.data, tok.ctypes.data, grp.ctypes.data)
    if rc < 0:
        raise HerroError(int(rc), "herro_debug_tile_plan_sib")
    nb, n64, n32 = (int(x) for x in n_tiles)
    return nb, n64, n32, order[:len(c)], tok[:nb + n64 + n32 + 1], grp[:nb]


def debug_launch_plan(nsup, Lf, tgt_win_off, batch_size: int, batch_mode: int = 0, fused: bool = True, fused_rows: int = 512,
                      packed: bool = True, qmode: int = 1, n_cu: int = 256):
    """The launch plan of herro_job_infer for a job of such windows (host only, herro_debug_launch_plan):
    (number of launches, launch of each window or 0xffffffff, its position in that launch's window stream, its padding length)."""
    ns, lf = np.ascontiguousarray(nsup, np.uint32), np.ascontiguousarray(Lf, np.uint32)
    two = np.ascontiguousarray(tgt_win_off, np.uint32)
    assert len(ns) == len(lf) and len(two) >= 1
    launch, pos, lmax = (np.zeros(max(len(ns), 1), np.uint32) for _ in range(3))
    n = lib().herro_debug_launch_plan(ns.ctypes.data, lf.ctypes.data, len(ns), two.ctypes.data, len(two) - 1, batch_size, batch_mode, int(fused), fused_rows,
                                      int(packed) | (qmode << 1), n_cu, launch.ctypes.data, pos.ctypes.data, lmax.ctypes.data)
    if n < 0:
        raise HerroError(int(n), "herro_debug_launch_plan")
    return int(n), launch[:len(ns)], pos[:len(ns)], lmax[:len(ns)]


FrontPlan = collections.namedtuple("FrontPlan", "fused fc_rows fc_grid conv_grid conv_units")


def debug_front_end_plan(n_tok: int, n_cu: int = 256, mode: int = -1) -> FrontPlan:
    """The front end of a launch of n_tok tokens on n_cu compute units (host only, herro_debug_front_end_plan; csrc/infer_plan.h front_end_plan):
    fused — k_conv_fc on fc_grid tiles of fc_rows tokens; else k_conv_m on conv_grid workgroups over conv_units blocks of 16 pairs, then k_fc_r on
    fc_grid tiles of fc_rows rows.  mode: -1 the selection rule, 0 two kernels, 1 k_conv_fc."""
    out = debug_front_end_plans(n_tok, 1, n_cu, mode)[0]
    return FrontPlan(bool(out[0]), *(int(x) for x in out[1:]))


def debug_front_end_plans(n_tok: int, count: int, n_cu: int = 256, mode: int = -1) -> np.ndarray:
    """... of the launches of n_tok, n_tok + 1, ... n_tok + count - 1 tokens: [count, 5] u32, the columns in FrontPlan's order"""
    out = np.zeros((max(count, 1), 5), np.uint32)
    rc = lib().herro_debug_front_end_plan(n_tok, count, n_cu, mode, out.ctypes.data)
    if rc < 0:
        raise HerroError(int(rc), "herro_debug_front_end_plan")
    return out[:count]


class Pool:
    """herro_pool (csrc/pool.cpp): several contexts of one process fed from one queue of target groups — the in-process layout of
    lib.rs:154-200.  device_ids: one entry per context (several may name the same GPU: they share its read store)."""

    def __init__(self, device_ids, fake_us_per_aln=None):
        """fake_us_per_aln: test hook (herro_debug_pool_fake) — a device-free pool of len(fake_us_per_aln) stand-in contexts."""
        self._l = lib()
        if fake_us_per_aln is not None:
            us = np.ascontiguousarray(fake_us_per_aln, np.uint32)
            self.h = self._l.herro_debug_pool_fake(len(us), us.ctypes.data)
            self.n = len(us)
            if not self.h:
                raise HerroError(-1, "herro_debug_pool_fake")
            return
        ids = (C.c_int * len(device_ids))(*device_ids)
        self.h = self._l.herro_pool_create(ids, len(device_ids))
        if not self.h:
            raise HerroError(-1, self._l.herro_last_error(None).decode(errors="replace"))
        self.n = len(device_ids)

    def skipped(self) -> tuple[int, int]:
        a, t = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._l.herro_pool_skipped(self.h, C.byref(a), C.byref(t)))
        return a.value, t.value

    def _chk(self, rc):
        if rc < 0:
            raise HerroError(int(rc), self._l.herro_pool_last_error(self.h).decode(errors="replace"))
        return rc

    def set_reads(self, seq, qual, off, name_class=None):
        seq, qual, off = np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(qual, np.uint8), np.ascontiguousarray(off, np.uint64)
        nc = None if name_class is None else np.ascontiguousarray(name_class, np.uint32)
        self._chk(self._l.herro_pool_set_reads(self.h, len(off) - 1, seq.ctypes.data, qual.ctypes.data, off.ctypes.data, None if nc is None else nc.ctypes.data))

    def load_model(self, path: str):
        self._chk(self._l.herro_pool_load_model(self.h, path.encode()))

    def set_precision(self, mode: int):
        for i in range(self.n):
            rc = self._l.herro_set_precision(self._l.herro_pool_ctx(self.h, i), mode)
            if rc:
                raise HerroError(rc, self._l.herro_last_error(self._l.herro_pool_ctx(self.h, i)).decode(errors="replace"))

    def correct(self, rids, rows, aln_off, cig_blob, cig_off, window_size: int, batch: int, read_ids, batch_mode: int = 1, group_targets: int = 1024):
        """FASTA text (u8 array) of all targets in target order + the end offset of every target's records."""
        rids = np.ascontiguousarray(rids, np.uint32)
        aln_off = np.ascontiguousarray(aln_off, np.uint64)
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 10)
        blob = np.ascontiguousarray(cig_blob, np.uint8)
        m = len(rows)
        raw = np.zeros((max(m, 1), 12), np.uint32)            # herro_alignment: 10 u32 + the CIGAR pointer
        if m:
            raw[:m, :10] = rows
            raw[:m, 10:12] = (np.asarray(cig_off, np.uint64) + np.uint64(blob.ctypes.data)).view(np.uint32).reshape(m, 2)
        names = (C.c_char_p * max(len(read_ids), 1))(*[r if isinstance(r, bytes) else r.encode() for r in read_ids])
        if len(read_ids) != len(rids):
            raise ValueError("one read id per target")
        n = self._chk(self._l.herro_pool_correct(self.h, len(rids), rids.ctypes.data, aln_off.ctypes.data, raw.ctypes.data, window_size, batch, batch_mode,
                                                 group_targets, names, None))
        ends_p = C.c_void_p()
        tp = self._l.herro_pool_result(self.h, C.byref(ends_p))
        text = np.ctypeslib.as_array((C.c_uint8 * n).from_address(tp)).copy() if n else np.zeros(0, np.uint8)
        ends = np.ctypeslib.as_array((C.c_uint64 * len(rids)).from_address(ends_p.value)).copy() if len(rids) else np.zeros(0, np.uint64)
        return text, ends

    def groups_taken(self):
        return [int(self._l.herro_pool_groups_taken(self.h, i)) for i in range(self.n)]

    def close(self):
        if self.h:
            self._l.herro_pool_destroy(self.h)
            self.h = None


@dataclass
class Window:
    info: WindowInfo
    bases: np.ndarray     # u8 [L',31]
    quals: np.ndarray     # u8 [L',31]
    sup_pos: np.ndarray   # u16
    sup_ins: np.ndarray   # u8
    qids: np.ndarray      # u32 ranked overlap ids


class Context:
    last_occ_cut = None   # the frequency cut of the latest find_overlaps

    def __init__(self, device: int = 0):
        self._l = lib()
        self.h = self._l.herro_create(device)
        if not self.h:
            raise HerroError(-2, self._l.herro_last_error(None).decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None):
            self._l.herro_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc: int):
        if rc != 0:
            raise HerroError(rc, self._l.herro_last_error(self.h).decode(errors="replace"))

    def last_error(self) -> str:
        return self._l.herro_last_error(self.h).decode(errors="replace")

    def set_stream(self, hip_stream: int | None):
        self._chk(self._l.herro_set_stream(self.h, hip_stream))

    def synchronize(self):
        self._chk(self._l.herro_synchronize(self.h))

    def set_reads(self, seq: np.ndarray, qual: np.ndarray, off: np.ndarray, name_class: np.ndarray | None = None):
        seq = np.ascontiguousarray(seq, np.uint8)
        qual = np.ascontiguousarray(qual, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        nc = None if name_class is None else np.ascontiguousarray(name_class, np.uint32)
        self._chk(self._l.herro_set_reads(self.h, len(off) - 1, seq.ctypes.data, qual.ctypes.data, off.ctypes.data,
                                          None if nc is None else nc.ctypes.data))
        self.n_reads = len(off) - 1

    def share_reads(self, other: "Context"):
        """Adopt the read store of another context of the same device (herro_share_reads): one copy in HBM per device."""
        self._chk(self._l.herro_share_reads(self.h, other.h))
        self.n_reads = getattr(other, "n_reads", None)

    def cut_store(self, pieces, name_class: np.ndarray | None = None):
        """Replace the read store by pieces of it, on the device (herro_store_cut): read x of the new store is bases [start, end) of read rid of
        the current one, in the order of `pieces` (PIECE_DTYPE, as trim_plan returns them).  What io.cut_reads + set_reads build, without a base
        crossing PCIe."""
        pieces = np.ascontiguousarray(pieces, PIECE_DTYPE)
        nc = None if name_class is None else np.ascontiguousarray(name_class, np.uint32)
        if nc is not None and len(nc) != len(pieces):
            raise HerroError(-1, "herro_store_cut: name_class has one entry per piece")
        self._chk(self._l.herro_store_cut(self.h, len(pieces), pieces.ctypes.data, None if nc is None else nc.ctypes.data))
        self.n_reads = len(pieces)

    STORE_ARRAYS = (("words", np.uint64), ("word_off", np.uint64), ("qual", np.uint8), ("qual_off", np.uint64), ("p0", np.uint32), ("p1", np.uint32))

    def store_arrays(self) -> dict:
        """Test hook (herro_debug_store_copy): the six arrays of the read store as they lie on the device — words (the pad word included),
        word_off, qual (without its pad), qual_off, p0, p1 (their two pad entries included)."""
        out = {}
        for which, (name, dt) in enumerate(self.STORE_ARRAYS):
            nb = int(self._l.herro_debug_store_copy(self.h, which, None, 0))
            if nb < 0:
                self._chk(nb)
            a = np.zeros(nb // np.dtype(dt).itemsize, dt)
            got = int(self._l.herro_debug_store_copy(self.h, which, a.ctypes.data, a.nbytes))
            if got < 0:
                self._chk(got)
            out[name] = a
        return out

    def debug_scan_u32(self, values):
        """Test hook (herro_debug_scan_u32): the front end's exclusive scan of u32 on `values` -> (out u32 [n + 1], guard_hits)."""
        v = np.ascontiguousarray(values, np.uint32).reshape(-1)
        out, hits = np.zeros(len(v) + 1, np.uint32), C.c_uint32(0xFFFFFFFF)
        self._chk(self._l.herro_debug_scan_u32(self.h, v.ctypes.data if len(v) else None, len(v), out.ctypes.data, C.byref(hits)))
        return out, int(hits.value)

    def debug_radix_sort(self, keys, pays, shifts):
        """Test hook (herro_debug_radix_sort): the front end's stable LSD radix sort by the 8-bit digits at `shifts` -> (keys, pays, guard_hits),
        copies of the arrays (*k0, *p0) name afterwards."""
        k, p = np.array(keys, np.uint64).reshape(-1), np.array(pays, np.uint64).reshape(-1)
        if len(k) != len(p):
            raise ValueError("one payload per key")
        sh, hits = np.ascontiguousarray(shifts, np.uint32).reshape(-1), C.c_uint32(0xFFFFFFFF)
        self._chk(self._l.herro_debug_radix_sort(self.h, k.ctypes.data if len(k) else None, p.ctypes.data if len(k) else None, len(k),
                                                 sh.ctypes.data if len(sh) else None, len(sh), C.byref(hits)))
        return k, p, int(hits.value)

    def debug_offsets64(self, nbytes):
        """Test hook (herro_debug_offsets64): the device FASTA's 64-bit offsets of pieces of `nbytes` bytes -> (off u64 [n + 1], guard_hits)."""
        b = np.ascontiguousarray(nbytes, np.uint64).reshape(-1)
        off, hits = np.zeros(len(b) + 1, np.uint64), C.c_uint32(0xFFFFFFFF)
        self._chk(self._l.herro_debug_offsets64(self.h, b.ctypes.data if len(b) else None, len(b), off.ctypes.data, C.byref(hits)))
        return off, int(hits.value)

    def load_model(self, path: str):
        self._chk(self._l.herro_load_model(self.h, path.encode()))

    def set_precision(self, mode: int):
        self._chk(self._l.herro_set_precision(self.h, mode))

    def precision(self) -> int:
        """the mode in force: the caller's, or the tier herro_load_model's calibration chose"""
        return int(self._l.herro_precision(self.h))

    def calibration_error(self, mode: int) -> float:
        """max |logit(mode) - logit(mode 0)| on the load-time calibration batch (-1: not measured)"""
        return float(self._l.herro_calibration_error(self.h, mode))

    def clock_probe(self) -> float:
        """shader clock in MHz right behind the work queued on this context's stream (herro_clock_probe; synchronises the stream)"""
        v = C.c_double(0.0)
        self._chk(self._l.herro_clock_probe(self.h, C.byref(v)))
        return float(v.value)

    def force_precision(self, on: bool):
        """test hook (herro_debug_force_precision): set_precision / load_model skip the calibration gate"""
        self._chk(self._l.herro_debug_force_precision(self.h, int(on)))

    def job_arrays(self, job: "Job") -> dict:
        out = {}
        for which, (name, dt) in enumerate([("ops", np.dtype("<u4")), ("ow", OW_DTYPE), ("win", WIN_DTYPE), ("tile_win", np.dtype("<u4")),
                                            ("tile_r0", np.dtype("<u4")), ("tgt_win_off", np.dtype("<u4"))]):
            p, eb = C.c_void_p(), C.c_uint32()
            n = self._l.herro_debug_job_array(job.h, which, C.byref(p), C.byref(eb))
            assert n >= 0 and eb.value == dt.itemsize, (name, n, eb.value, dt.itemsize)
            out[name] = np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(p.value), dt, n).copy() if n else np.zeros(0, dt)
        return out

    def host_build(self, on: bool):
        """test hook: jobs created from now on are windowed / described by the host (rounds 3-5) instead of on the device (build_dev.hip)"""
        self._chk(self._l.herro_debug_set_host_build(self.h, int(on)))

    def featurize_planes(self, on: bool):
        """test hook: jobs featurized from now on take the planes path (k_tokens) instead of the lean one (k_rows)"""
        self._chk(self._l.herro_debug_set_featurize_planes(self.h, int(on)))

    def conv_fc(self, mode: int):
        """test hook: front end of the f16 model from now on: -1 chosen per launch, 0 k_conv_m + k_fc_r, 1 k_conv_fc wherever its shapes allow"""
        self._chk(self._l.herro_debug_set_conv_fc(self.h, int(mode)))

    def front_cu(self, n_cu: int):
        """test hook: the front end (conv stack + FC projection) plans its launches for n_cu compute units from now on, 0 the device's own;
        the encoder stack's tile plan keeps the device's count"""
        self._chk(self._l.herro_debug_set_front_cu(self.h, int(n_cu)))

    def front_last(self) -> "FrontPlan":
        """test hook: what the front end of this context's last model launch sent out"""
        out = np.zeros(5, np.uint32)
        self._chk(self._l.herro_debug_front_last(self.h, out.ctypes.data))
        return FrontPlan(bool(out[0]), *(int(x) for x in out[1:]))

    def register_host(self, arr: np.ndarray):
        """herro_host_register: jobs whose CIGAR pointers lie in `arr` (a contiguous u8 array the caller keeps alive) are created zero-copy."""
        self._chk(self._l.herro_host_register(self.h, arr.ctypes.data, arr.nbytes))

    def unregister_host(self, arr: np.ndarray):
        self._chk(self._l.herro_host_unregister(self.h, arr.ctypes.data))

    def describe_model(self) -> str:
        buf = C.create_string_buffer(4096)
        n = self._l.herro_model_describe(self.h, buf, 4096)
        if n < 0:
            self._chk(int(n))
        return buf.value.decode()

    def create_job(self, rids, aln_rows: np.ndarray, aln_off, cigars: list[bytes] | None, window_size: int,
                   cig_blob: np.ndarray | None = None, cig_off: np.ndarray | None = None) -> "Job":
        """aln_rows u32 [n,>=9] (qid,qlen,qstart,qend,strand,tid,tlen,tstart,tend[,cigar_len]); CIGARs either
        as a list of bytes or as blob + offsets (+ lengths in column 9)."""
        rids = np.ascontiguousarray(rids, np.uint32)
        aln_off = np.ascontiguousarray(aln_off, np.uint64)
        n = len(aln_rows)
        if cigars is not None:
            lens = np.array([len(c) for c in cigars], np.uint64)
            cig_off = np.zeros(n, np.uint64)
            if n:
                cig_off[1:] = np.cumsum(lens)[:-1]
            cig_blob = np.frombuffer(b"".join(cigars) + b"\0", np.uint8).copy()
            cl = lens
        else:
            cig_blob = np.ascontiguousarray(cig_blob, np.uint8)
            cl = aln_rows[:, 9].astype(np.uint64)
        arr, view = _aln_array(aln_rows)
        if n:
            view["f"][:n, 9] = cl
            view["p"][:n] = cig_blob.ctypes.data + np.asarray(cig_off, np.uint64)
        h = self._l.herro_job_create(self.h, len(rids), rids.ctypes.data, aln_off.ctypes.data, C.byref(arr), window_size)
        return _job_or_raise(self, h, len(rids))

    def align(self, rows: np.ndarray):
        """Base-level alignment of overlaps given by coordinates only (herro_align_overlaps; the `minimap2 -c` step of mm2.rs:15-30
        plus fix_cigar, aligners.rs:138-250).  rows: u32 [n, >=9] in create_job's layout (qid, qlen, qstart, qend, strand, tid, tlen,
        tstart, tend).  Returns (rows_out u32 [n, 10] with the trimmed coordinates and the CIGAR lengths, cigars: list of bytes,
        scores: i32 [n], ok: bool [n]); a failed record keeps its coordinates and gets an empty CIGAR."""
        rows = np.ascontiguousarray(rows, np.uint32)
        n = len(rows)
        arr, _ = _aln_array(rows)
        h = C.c_void_p()
        self._chk(self._l.herro_align_overlaps(self.h, n, C.byref(arr), C.byref(h)))
        try:
            out, ptr = _aln_rows(self._l.herro_aligned_alignments(h), n, with_cigar_ptr=True)
            scores = np.zeros(n, np.int32)
            if n:
                scores[:] = np.ctypeslib.as_array(C.cast(self._l.herro_aligned_scores(h), C.POINTER(C.c_int32)), (n,))
            cigars = [C.string_at(int(p), int(k)) if k else b"" for p, k in zip(ptr, out[:, 9])]
        finally:
            self._l.herro_aligned_free(h)
        return out, cigars, scores, out[:, 9] > 0

    def align_dev(self, rows: np.ndarray) -> "AlignedDev":
        """Context.align with the ops left on the device (herro_align_overlaps_dev): a handle for create_job_aligned.  No CIGAR text
        exists unless AlignedDev.cigar asks for one."""
        rows = np.ascontiguousarray(rows, np.uint32)
        n = len(rows)
        arr, _ = _aln_array(rows)
        h = C.c_void_p()
        self._chk(self._l.herro_align_overlaps_dev(self.h, n, C.byref(arr), C.byref(h)))
        return AlignedDev(self, h)

    def aligned_dev_from_ops(self, rows: np.ndarray, op_off, ops) -> "AlignedDev":
        """A handle over the caller's binary CIGARs (herro_aligned_dev_from_ops): record r has ops[op_off[r] : op_off[r + 1]], each
        len << 2 | (0 M, 1 I, 2 D); rows as for align, taken as given."""
        rows = np.ascontiguousarray(rows, np.uint32)
        op_off = np.ascontiguousarray(op_off, np.uint64)
        ops = np.ascontiguousarray(ops, np.uint32)
        n = len(rows)
        if len(op_off) != n + 1 or (n and int(op_off[-1]) > len(ops)):
            raise ValueError("op_off has one entry per record + 1 and ends inside ops")
        arr, _ = _aln_array(rows)
        h = C.c_void_p()
        self._chk(self._l.herro_aligned_dev_from_ops(self.h, n, C.byref(arr), op_off.ctypes.data, ops.ctypes.data if len(ops) else None, C.byref(h)))
        return AlignedDev(self, h)

    def create_job_aligned(self, rids, aln_off, rec, handle: "AlignedDev", window_size: int) -> "Job":
        """herro_job_create_aligned: target t's alignments are records rec[aln_off[t] : aln_off[t + 1]] of `handle` (aligned_dev_job_args
        makes the three from find_overlaps' grouping).  The handle may be closed as soon as this returns."""
        rids = np.ascontiguousarray(rids, np.uint32)
        aln_off = np.ascontiguousarray(aln_off, np.uint64)
        rec = np.ascontiguousarray(rec, np.uint32)
        if len(aln_off) != len(rids) + 1 or (len(rids) and int(aln_off[-1]) > len(rec)):
            raise ValueError("aln_off has one entry per target + 1 and ends inside rec")
        h = self._l.herro_job_create_aligned(self.h, len(rids), rids.ctypes.data, aln_off.ctypes.data, rec.ctypes.data if len(rec) else None,
                                             handle.h, window_size)
        return _job_or_raise(self, h, len(rids))

    def _overlap_params(self, params: dict) -> OverlapParams:
        """keyword arguments -> herro_overlap_params.  A field left out (or None) takes its default, which the struct spells 0; an
        explicit k or w outside 5 .. 31 / 1 .. 64 — 0 included, which the struct could not carry — is HERRO_E_INVALID here.
        occ_frac_ppm (0 or left out: the fixed cut max_occ): the cut is taken from the store's index so that at most this many parts per
        million of the distinct minimizers lie above it (minimap2's -f; 5000 = the reference's -f0.005), max_occ becomes its ceiling
        (0: none); values outside 0 .. 999999 are the library's HERRO_E_INVALID."""
        p = OverlapParams()
        for name, v in params.items():
            if name not in ("k", "w", "max_occ", "bandwidth", "max_gap", "min_score", "min_anchors", "occ_frac_ppm"):
                raise TypeError(f"unknown overlap parameter {name!r}")
            if v is None:
                continue
            v = int(v)
            if (name == "k" and not 5 <= v <= 31) or (name == "w" and not 1 <= v <= 64) or not 0 <= v <= 0xFFFFFFFF:
                raise HerroError(-1, "overlap parameters: 5 <= k <= 31 and 1 <= w <= 64")
            setattr(p, name, v)
        return p

    def _core_mask(self, core):
        """a core mask as the library takes it: u8 [n_reads], non-zero = the read is a target.  Its length must be the store's read count."""
        m = np.ascontiguousarray(core)
        m = np.ascontiguousarray(m, np.uint8) if m.dtype == np.uint8 else np.ascontiguousarray(m != 0, np.uint8)
        n = getattr(self, "n_reads", None)   # (None: no reads yet — the call answers HERRO_E_STATE)
        if m.ndim != 1 or (n is not None and len(m) != n):
            raise ValueError(f"core has shape {m.shape}, the read store {n} reads")
        return m

    def set_seed_rescue(self, occ_dist: int | None = 200, rescue_max_occ: int | None = None):
        """The rescue of high-frequency minimizers for every later find_overlaps / find_overlap_pairs of this context (herro_set_seed_rescue;
        minimap2's -e, the reference's -e200: mm2.rs:24): of a stretch of a read whose minimizers all lie above the frequency cut the least
        frequent ones stay, about one per occ_dist bases, among the hashes of at most rescue_max_occ (None / 0: 4095) occurrences.
        occ_dist None or 0: off.  Values outside 0 .. 2^20 / 0 .. 65534 are the library's HERRO_E_INVALID."""
        d, m = int(occ_dist or 0), int(rescue_max_occ or 0)
        if not 0 <= d <= 0xFFFFFFFF or not 0 <= m <= 0xFFFFFFFF:
            raise HerroError(-1, "seed rescue: occ_dist and rescue_max_occ are unsigned 32-bit values")
        p = SeedRescueParams(occ_dist=d, rescue_max_occ=m)
        self._chk(self._l.herro_set_seed_rescue(self.h, C.byref(p) if d or m else None))
        self._seed_rescue = (d, m)

    @contextlib.contextmanager
    def _rescue_keywords(self, params: dict):
        """occ_dist= / rescue_max_occ= of one finder call: taken out of params, set for the call, the context's setting restored behind it"""
        if "occ_dist" not in params and "rescue_max_occ" not in params:
            yield
            return
        before = getattr(self, "_seed_rescue", (0, 0))
        d, m = params.pop("occ_dist", before[0]), params.pop("rescue_max_occ", before[1])
        self.set_seed_rescue(d, m)
        try:
            yield
        finally:
            self.set_seed_rescue(*before)

    def set_chain_lookback(self, n: int | None = 0):
        """The predecessors a chain step of every later find_overlaps / find_overlap_pairs of this context looks at (herro_set_chain_params;
        minimap2's max_chain_iter): a multiple of 64 in 64 .. 1024; None or 0: 64, the default, which runs the kernels that always ran.  A
        tandem repeat whose anchors survive the frequency cut breaks a chain at 64; DESIGN.md section 10, "A longer look-back".  Any other
        value is the library's HERRO_E_INVALID, and the setting stays as it was."""
        n = int(n or 0)
        if not 0 <= n <= 0xFFFFFFFF:
            raise HerroError(-1, "chain look-back: an unsigned 32-bit value")
        p = ChainParams(lookback=n)
        self._chk(self._l.herro_set_chain_params(self.h, C.byref(p)))
        self._chain_lookback = n or 64

    @property
    def chain_lookback(self) -> int:
        """the look-back in force (set_chain_lookback; 64 unless set)"""
        return getattr(self, "_chain_lookback", 64)

    @contextlib.contextmanager
    def _chain_keywords(self, params: dict):
        """lookback= of one finder call: taken out of params, set for the call, the context's setting restored behind it"""
        if "lookback" not in params:
            yield
            return
        before = self.chain_lookback
        n = params.pop("lookback")
        self.set_chain_lookback(before if n is None else n)
        try:
            yield
        finally:
            self.set_chain_lookback(before)

    def set_index_parts(self, max_kmers: int | None = None, occ_ranges: int = 0):
        """The index of every later find_overlaps / find_overlap_pairs of this context in parts of at most max_kmers k-mers (herro_set_index_params;
        minimap2's -I): the store may then hold more than 2^32 k-mers, and the index arrays are those of one part.  The result is byte for byte the
        unpartitioned call's for every max_kmers.  occ_ranges: the hash ranges of the occurrence pass, 0: chosen by the library.  max_kmers None or
        0: off, the default, which runs the kernels that always ran.  max_kmers > 2^32 - 4096 or occ_ranges > 65536 is the library's
        HERRO_E_INVALID, and the setting stays as it was.  DESIGN.md section 10, "An index in parts"."""
        m, r = int(max_kmers or 0), int(occ_ranges or 0)
        if not 0 <= m <= 0xFFFFFFFFFFFFFFFF or not 0 <= r <= 0xFFFFFFFF:
            raise HerroError(-1, "index parts: max_kmers is an unsigned 64-bit value, occ_ranges an unsigned 32-bit one")
        p = IndexParams(max_kmers=m, occ_ranges=r)
        self._chk(self._l.herro_set_index_params(self.h, C.byref(p) if m or r else None))
        self._index_parts = (m, r)

    @contextlib.contextmanager
    def _index_keywords(self, params: dict):
        """index_kmers= / occ_ranges= of one finder call: taken out of params, set for the call, the context's setting restored behind it"""
        if "index_kmers" not in params and "occ_ranges" not in params:
            yield
            return
        before = getattr(self, "_index_parts", (0, 0))
        m, r = params.pop("index_kmers", before[0]), params.pop("occ_ranges", before[1])
        self.set_index_parts(m, r)
        try:
            yield
        finally:
            self.set_index_parts(*before)

    def chain(self, groups, **params):
        """Test hook (herro_debug_chain): the chain stage alone under the context's look-back, or the lookback= given here.  groups: a list of
        (tpos, qpos) array pairs, each not empty and strictly ascending by (tpos, qpos) with coordinates below 2^31; params: k, bandwidth,
        max_gap.  Returns i32 [n_groups, 4]: score, first anchor, last anchor, anchors in the chain — tests/overlap_ref.py::chain."""
        tps = [np.ascontiguousarray(t, np.uint32).reshape(-1) for t, _ in groups]
        qps = [np.ascontiguousarray(q, np.uint32).reshape(-1) for _, q in groups]
        if any(len(t) != len(q) for t, q in zip(tps, qps)):
            raise ValueError("one qpos per tpos")
        off = np.zeros(len(tps) + 1, np.uint64)
        off[1:] = np.cumsum([len(t) for t in tps])
        tp = np.concatenate(tps) if tps else np.zeros(0, np.uint32)
        qp = np.concatenate(qps) if qps else np.zeros(0, np.uint32)
        out = np.zeros((len(tps), 4), np.int32)
        with self._chain_keywords(params):
            p = self._overlap_params(params)
            self._chk(self._l.herro_debug_chain(self.h, len(tps), off.ctypes.data, tp.ctypes.data if len(tp) else None,
                                                qp.ctypes.data if len(qp) else None, C.byref(p), out.ctypes.data if len(tps) else None))
        return out

    def seed_rescue(self, **params):
        """The rescue alone (herro_debug_seed_rescue) under the context's setting, or the occ_dist= / rescue_max_occ= given here: for the
        minimizers in sketch()'s order, (occ u32 = min(occurrences of the hash in the store, 65535), rescued u8).  index_kmers= / occ_ranges=:
        set_index_parts for this call alone — occ then comes from the occurrence pass over hash ranges, the rescue runs block by block."""
        with self._rescue_keywords(params), self._index_keywords(params):
            p = self._overlap_params(params)
            n = self._l.herro_debug_seed_rescue(self.h, C.byref(p), None, None, 0)
            if n < 0:
                self._chk(int(n))
            occ, resc = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            if n:
                got = self._l.herro_debug_seed_rescue(self.h, C.byref(p), occ.ctypes.data, resc.ctypes.data, n)
                if got < 0:
                    self._chk(int(got))
                assert got == n
        return occ, resc

    def find_overlaps(self, core=None, **params):
        """Which reads of the store overlap, where, on which strand (herro_find_overlaps; the seeding and chaining of the
        `minimap2 -x ava-ont` run of mm2.rs:15-30).  params: k, w, max_occ, bandwidth, max_gap, min_score, min_anchors, occ_frac_ppm, and
        occ_dist / rescue_max_occ: set_seed_rescue for this call alone (the minimizers it rescued are left in self.last_rescued);
        lookback: set_chain_lookback for this call alone; index_kmers / occ_ranges: set_index_parts for this call alone (the read blocks of
        the call are left in self.last_index_blocks, 0: the setting was off).
        The frequency cut the call used (max_occ, or the one occ_frac_ppm gave) is left in self.last_occ_cut.
        Returns (rids u32 [n_targets], rows u32 [n, 10] in create_job's layout with cigar_len 0, aln_off u64 [n_targets + 1],
        scores i32 [n]): rows goes into Context.align, (rids, aln_off) with its result into aligned_job_args.
        core: u8 [n_reads], non-zero = the read is a target (herro_find_overlaps_core): the records whose tid is core; None: all."""
        h = C.c_void_p()
        with self._rescue_keywords(params), self._chain_keywords(params), self._index_keywords(params):   # (each set for this call alone)
            p = self._overlap_params(params)
            if core is None:
                self._chk(self._l.herro_find_overlaps(self.h, C.byref(p), C.byref(h)))
            else:
                m = self._core_mask(core)
                self._chk(self._l.herro_find_overlaps_core(self.h, C.byref(p), m.ctypes.data, C.byref(h)))
        try:
            n, nt = self._l.herro_overlaps_n(h), self._l.herro_overlaps_n_targets(h)
            if hasattr(self._l, "herro_overlaps_occ_cut"):
                self.last_occ_cut = int(self._l.herro_overlaps_occ_cut(h))
            if hasattr(self._l, "herro_overlaps_rescued"):
                self.last_rescued = int(self._l.herro_overlaps_rescued(h))
            if hasattr(self._l, "herro_overlaps_index_blocks"):
                self.last_index_blocks = int(self._l.herro_overlaps_index_blocks(h))
            rids = np.ctypeslib.as_array(C.cast(self._l.herro_overlaps_target_ids(h), C.POINTER(C.c_uint32)), (nt,)).copy() if nt else np.zeros(0, np.uint32)
            aln_off = np.ctypeslib.as_array(C.cast(self._l.herro_overlaps_aln_off(h), C.POINTER(C.c_uint64)), (nt + 1,)).copy()
            rows = _aln_rows(self._l.herro_overlaps_alignments(h), n)
            scores = np.zeros(n, np.int32)
            if n:
                scores[:] = np.ctypeslib.as_array(C.cast(self._l.herro_overlaps_scores(h), C.POINTER(C.c_int32)), (n,))
        finally:
            self._l.herro_overlaps_free(h)
        return rids, rows, aln_off, scores

    def extend_overlaps(self, rows: np.ndarray, zdrop: int = 0, max_ext: int = 0):
        """Extends coordinate-only overlaps to where the reads stop agreeing (herro_extend_overlaps): the step between
        find_overlaps and align / align_dev.  rows: u32 [n, >=9] as find_overlaps returns and align takes; zdrop, max_ext: 0 = the defaults
        (400, 2048).  Returns (rows_out u32 [n, 10] with the extended coordinates and cigar_len 0, ext u32 [n, 4]: bases gained as t_left,
        q_left, t_right, q_right — the q lengths on the oriented query —, scores i32 [n, 2]: left, right)."""
        rows = np.ascontiguousarray(rows, np.uint32)
        n = len(rows)
        if not 0 <= int(zdrop) <= 0xFFFFFFFF or not 0 <= int(max_ext) <= 0xFFFFFFFF:
            raise HerroError(-1, "extend parameters: zdrop and max_ext are unsigned 32-bit values")
        arr, _ = _aln_array(rows)
        p = ExtendParams(zdrop=int(zdrop), max_ext=int(max_ext))
        h = C.c_void_p()
        self._chk(self._l.herro_extend_overlaps(self.h, n, C.byref(arr), C.byref(p), C.byref(h)))
        try:
            assert self._l.herro_extended_n(h) == n
            out = _aln_rows(self._l.herro_extended_alignments(h), n)
            ext = np.zeros((n, 4), np.uint32)
            scores = np.zeros((n, 2), np.int32)
            if n:
                ext[:] = np.ctypeslib.as_array(C.cast(self._l.herro_extended_ext(h), C.POINTER(C.c_uint32)), (n, 4))
                scores[:] = np.ctypeslib.as_array(C.cast(self._l.herro_extended_scores(h), C.POINTER(C.c_int32)), (n, 2))
        finally:
            self._l.herro_extended_free(h)
        return out, ext, scores

    def find_adapters(self, adapters, max_err_pm: int = 0, forward_only: bool = False):
        """Approximate matches of every adapter in every read of the store, both strands (herro_find_adapters): adapters = byte strings of 8 .. 64
        bases ACGT, at most 32; up to floor(len * max_err_pm / 1000) errors (0: 250, at most 500); forward_only: strand 0 alone.
        Returns (hits ADAPTER_HIT_DTYPE ascending (rid, end, start, adapter, strand), hits_off u64 [n_reads + 1]): the arguments of trim_plan."""
        adapters = [bytes(a) for a in adapters]
        if not 0 <= int(max_err_pm) <= 0xFFFFFFFF:
            raise HerroError(-1, "herro_find_adapters: max_err_pm is an unsigned 32-bit value")
        off = np.zeros(len(adapters) + 1, np.uint64)
        off[1:] = np.cumsum([len(a) for a in adapters])
        p = AdapterParams(max_err_pm=int(max_err_pm), flags=ADAPTERS_FORWARD_ONLY if forward_only else 0)
        h = C.c_void_p()
        self._chk(self._l.herro_find_adapters(self.h, len(adapters), b"".join(adapters), off.ctypes.data, C.byref(p), C.byref(h)))
        try:
            n = int(self._l.herro_adapter_hits_n(h))
            hits = np.zeros(n, ADAPTER_HIT_DTYPE)
            if n:
                C.memmove(hits.ctypes.data, self._l.herro_adapter_hits_data(h), hits.nbytes)
            hits_off = np.zeros(self.n_reads + 1, np.uint64)
            C.memmove(hits_off.ctypes.data, self._l.herro_adapter_hits_off(h), hits_off.nbytes)
        finally:
            self._l.herro_adapter_hits_free(h)
        return hits, hits_off

    def adapter_cap(self, cap: int):
        """Test hook (herro_debug_set_adapter_cap): the hits the first scan's buffer of every later find_adapters holds; 0: the default."""
        self._chk(self._l.herro_debug_set_adapter_cap(self.h, int(cap)))

    def fasta_chunk(self, nbytes: int):
        """Test hook (herro_debug_set_fasta_chunk): the text bytes of a chunk of every later Job.fasta_dev; 0: the default."""
        self._chk(self._l.herro_debug_set_fasta_chunk(self.h, int(nbytes)))

    def find_overlap_pairs(self, extend: bool = True, zdrop: int = 0, max_ext: int = 0, core=None, **params) -> "OverlapPairs":
        """find_overlaps, pair_rows, extend_overlaps over the primaries and paired_job_args' table in one call that keeps the records on the
        device (herro_find_overlap_pairs): one record per read pair and the table of the finder's two rows per pair.  params as
        find_overlaps; zdrop, max_ext as extend_overlaps; extend=False: HERRO_PAIRS_NO_EXTEND, the chains' anchor spans as they are.
        core: u8 [n_reads], non-zero = the read is a target (herro_find_overlap_pairs_core): only pairs with a core read are chained, extended
        and later aligned, and the table holds only the rows whose target is core — a selection of the unmasked handle; None: all reads."""
        if not 0 <= int(zdrop) <= 0xFFFFFFFF or not 0 <= int(max_ext) <= 0xFFFFFFFF:
            raise HerroError(-1, "extend parameters: zdrop and max_ext are unsigned 32-bit values")
        e = ExtendParams(zdrop=int(zdrop), max_ext=int(max_ext))
        h = C.c_void_p()
        flags = 0 if extend else PAIRS_NO_EXTEND
        with self._rescue_keywords(params), self._chain_keywords(params), self._index_keywords(params):   # (occ_dist= / rescue_max_occ= / lookback= / index_kmers= / occ_ranges=: set for this call alone)
            p = self._overlap_params(params)
            if core is None:
                self._chk(self._l.herro_find_overlap_pairs(self.h, C.byref(p), C.byref(e), flags, C.byref(h)))
            else:
                m = self._core_mask(core)
                self._chk(self._l.herro_find_overlap_pairs_core(self.h, C.byref(p), C.byref(e), flags, m.ctypes.data, C.byref(h)))
        return OverlapPairs(self, h)

    def pairs_from_table(self, primaries: np.ndarray, chain_scores, rids, aln_off, rec_of_row, n_rows: int | None = None) -> "OverlapPairs":
        """A handle over a table the caller built (herro_pairs_from_table; also on a HostContext): primaries u32 [P, >= 9] as rows[prim],
        chain_scores i32 [P] or None, (rids, aln_off) the grouping of the 2 P rows by target, rec_of_row as pair_rows returns it.
        n_rows: a table of core targets (herro_pairs_from_table_core) — n_rows <= 2 P rows, rec_of_row has n_rows entries."""
        rows = np.ascontiguousarray(primaries, np.uint32)
        n = len(rows)
        sc = None if chain_scores is None else np.ascontiguousarray(chain_scores, np.int32)
        rids = np.ascontiguousarray(rids, np.uint32)
        aln_off = np.ascontiguousarray(aln_off, np.uint64)
        rec_of_row = np.ascontiguousarray(rec_of_row, np.uint32)
        if len(aln_off) != len(rids) + 1 or len(rec_of_row) != (2 * n if n_rows is None else int(n_rows)) or (sc is not None and len(sc) != n):
            raise ValueError("aln_off has one entry per target + 1, rec_of_row two per primary (n_rows with n_rows), chain_scores one")
        arr, _ = _aln_array(rows)
        h = C.c_void_p()
        if n_rows is not None:
            self._chk(self._l.herro_pairs_from_table_core(self.h, n, C.byref(arr), None if sc is None else sc.ctypes.data, len(rids),
                                                          rids.ctypes.data if len(rids) else None, aln_off.ctypes.data, int(n_rows),
                                                          rec_of_row.ctypes.data if len(rec_of_row) else None, C.byref(h)))
            return OverlapPairs(self, h)
        self._chk(self._l.herro_pairs_from_table(self.h, n, C.byref(arr), None if sc is None else sc.ctypes.data, len(rids),
                                                 rids.ctypes.data if len(rids) else None, aln_off.ctypes.data,
                                                 rec_of_row.ctypes.data if n else None, C.byref(h)))
        return OverlapPairs(self, h)

    def cluster_graph(self, n_reads: int, a, b, n_parts: int, weights=None, span=None, min_span: int = 0) -> "Clusters":
        """herro_cluster_graph: the reads partitioned by an overlap graph given as arrays (also refused properly on a HostContext) — a, b u32 [E]
        the edges, span u32 [E] or None (every edge is strong), weights u32 [n_reads] or None (all 1), n_parts parts, edges with span < min_span
        weak.  The specification is include/herro_amd.h's, "clusters" (tests/cluster_ref.py)."""
        a, b = np.ascontiguousarray(a, np.uint32).reshape(-1), np.ascontiguousarray(b, np.uint32).reshape(-1)
        sp = None if span is None else np.ascontiguousarray(span, np.uint32).reshape(-1)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(-1)
        if len(b) != len(a) or (sp is not None and len(sp) != len(a)) or (w is not None and len(w) != int(n_reads)):
            raise ValueError("a, b and span have one entry per edge, weights one per read")
        if not 0 <= int(n_parts) <= 0xFFFFFFFF or not 0 <= int(min_span) <= 0xFFFFFFFF:
            raise HerroError(-1, "cluster parameters: n_parts and min_span are unsigned 32-bit values")
        P = ClusterParams(n_parts=int(n_parts), min_span=int(min_span))
        h = C.c_void_p()
        self._chk(self._l.herro_cluster_graph(self.h, int(n_reads), None if w is None else w.ctypes.data, len(a), a.ctypes.data if len(a) else None,
                                              b.ctypes.data if len(a) else None, None if sp is None else sp.ctypes.data, C.byref(P), C.byref(h)))
        return Clusters(self, h)

    def create_job_paired(self, pairs: "OverlapPairs", m: "AlignedDev", window_size: int) -> "Job":
        """herro_job_create_paired: create_job_aligned(*paired_job_args(pairs.rids, pairs.aln_off, pairs.rec_of_row, m.ok), m, window_size)
        inside the library; m: pairs.align() or any handle of 2 P records, primaries then mirrors."""
        h = self._l.herro_job_create_paired(self.h, pairs.h, m.h, window_size)
        return _job_or_raise(self, h, len(pairs.rids))

    def occ_census(self, **params):
        """The census and the pick of occ_frac_ppm alone (herro_debug_occ_census): (hist u32 [65536] over min(occurrences, 65535) of the
        distinct minimizer hashes, dict(cut, distinct, cut_runs, cut_minimizers)).  index_kmers= / occ_ranges=: set_index_parts for this call
        alone — the census is then the occurrence pass's, over hash ranges (a bin beyond 32 bits comes back as 2^32 - 1)."""
        hist, out = np.zeros(65536, np.uint32), np.zeros(4, np.uint64)
        with self._index_keywords(params):
            p = self._overlap_params(params)
            self._chk(self._l.herro_debug_occ_census(self.h, C.byref(p), hist.ctypes.data, out.ctypes.data))
        return hist, dict(zip(("cut", "distinct", "cut_runs", "cut_minimizers"), (int(x) for x in out)))

    def sketch(self, **params):
        """The store's minimizers sorted by (rid, pos) (herro_debug_sketch): (hash u64, rid u32, pos u32, strand u8)."""
        p = self._overlap_params(params)
        n = self._l.herro_debug_sketch(self.h, C.byref(p), None, None, None, None, 0)
        if n < 0:
            self._chk(int(n))
        hs, rid, pos, st = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        if n:
            got = self._l.herro_debug_sketch(self.h, C.byref(p), hs.ctypes.data, rid.ctypes.data, pos.ctypes.data, st.ctypes.data, n)
            if got < 0:
                self._chk(int(got))
            assert got == n
        return hs, rid, pos, st

    def create_job_from_paf(self, paf: "Paf", window_size: int) -> "Job":
        """herro_job_create straight from a parsed PAF batch (targets in its order); `paf` must outlive the call."""
        h = self._l.herro_job_create(self.h, len(paf.targets), paf.targets.ctypes.data, paf.aln_off.ctypes.data,
                                     paf._alns_ptr, window_size)
        return _job_or_raise(self, h, len(paf.targets))

    def model_forward(self, bases: np.ndarray, quals: np.ndarray, lens: np.ndarray, indices: np.ndarray):
        """inference.rs:147-175: tokens u8 [B,L,31], raw quals u8 [B,L,31], lens, flat indices -> logits."""
        bases = np.ascontiguousarray(bases, np.uint8)
        quals = np.ascontiguousarray(quals, np.uint8)
        lens = np.ascontiguousarray(lens, np.int32)
        indices = np.ascontiguousarray(indices, np.int32)
        B, L, R = bases.shape
        assert R == 31 and quals.shape == bases.shape
        N = int(lens.sum())
        info = np.zeros(N, np.float32)
        base = np.zeros((N, 5), np.float32)
        self._chk(self._l.herro_model_forward(self.h, B, L, bases.ctypes.data, quals.ctypes.data, lens.ctypes.data,
                                              indices.ctypes.data if N else None, info.ctypes.data, base.ctypes.data))
        return info, base

    def sib_fault(self):
        """test hook: what a sibling tile that timed out leaves behind (the next fetch repeats its job's model pass)"""
        self._chk(self._l.herro_debug_sib_fault(self.h))

    def sib_retries(self) -> int:
        return int(self._l.herro_debug_sib_retries(self.h))

    def timing_enable(self, on: bool = True):
        self._chk(self._l.herro_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._chk(self._l.herro_timing_reset(self.h))

    def timing(self) -> dict[str, tuple[float, int]]:
        n = C.c_uint32(256)
        names = C.create_string_buffer(8192)
        ms = (C.c_double * 256)()
        calls = (C.c_uint64 * 256)()
        self._chk(self._l.herro_timing_get(self.h, names, 8192, ms, calls, C.byref(n)))
        nm = [x for x in names.value.decode().split("\n") if x]
        return {nm[i]: (ms[i], int(calls[i])) for i in range(min(n.value, len(nm)))}


class Job:
    def __init__(self, ctx: Context, h, n_targets: int):
        self.ctx, self.h, self.n_targets = ctx, h, n_targets
        self._l = ctx._l

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self._l.herro_job_free(self.h)
        self.h = None

    __del__ = close

    @property
    def n_windows(self) -> int:
        return self._l.herro_job_n_windows(self.h)

    def skipped(self) -> tuple[int, int]:
        """(alignments left out, targets left without overlaps) — see herro_job_skipped"""
        a, t = C.c_uint32(0), C.c_uint32(0)
        self.ctx._chk(self._l.herro_job_skipped(self.h, C.byref(a), C.byref(t)))
        return a.value, t.value

    def featurize(self):
        self.ctx._chk(self._l.herro_job_featurize(self.h))

    def infer(self, batch_size: int, batch_mode: int = 0):
        self.ctx._chk(self._l.herro_job_infer(self.h, batch_size, batch_mode))

    def consensus(self):
        """consensus.rs:86-227 on the device; consensus_fasta() then only concatenates windows."""
        self.ctx._chk(self._l.herro_job_consensus(self.h))

    def consensus_fetch(self) -> int:
        """corrected bases of the whole job -> host; returns how many (herro_job_consensus_fetch)"""
        n = C.c_uint64(0)
        self.ctx._chk(self._l.herro_job_consensus_fetch(self.h, C.byref(n)))
        return n.value

    def info(self, w: int) -> WindowInfo:
        wi = WindowInfo()
        self.ctx._chk(self._l.herro_job_window_info(self.h, w, C.byref(wi)))
        return wi

    def window(self, w: int, encoded: bool = False) -> Window:
        wi = self.info(w)
        bases = np.zeros((wi.length, 31), np.uint8)
        quals = np.zeros((wi.length, 31), np.uint8)
        sp = np.zeros(wi.n_supported, np.uint16)
        si = np.zeros(wi.n_supported, np.uint8)
        qids = np.zeros(wi.n_overlaps, np.uint32)
        self.ctx._chk(self._l.herro_job_window_copy(self.h, w, int(encoded), bases.ctypes.data, quals.ctypes.data,
                                                    sp.ctypes.data, si.ctypes.data, qids.ctypes.data))
        return Window(wi, bases, quals, sp, si, qids)

    def logits(self, w: int):
        wi = self.info(w)
        info = np.zeros(wi.n_supported, np.float32)
        base = np.zeros((wi.n_supported, 5), np.float32)
        self.ctx._chk(self._l.herro_job_window_logits(self.h, w, info.ctypes.data, base.ctypes.data))
        return info, base

    def consensus_fasta(self, t: int, read_id: str, desc: str | None = None) -> str:
        cap = 1 << 24
        out = getattr(self, "_fasta_buf", None)
        if out is None:                     # one buffer per job: allocating (and zeroing) 16 MB per target dominated multi-target runs
            out = self._fasta_buf = C.create_string_buffer(cap)
        n = self._l.herro_job_consensus_fasta(self.h, t, read_id.encode(), None if desc is None else desc.encode(), out, cap)
        if n < 0:
            self.ctx._chk(int(n))
        return C.string_at(out, n).decode()   # (out.raw would copy the whole 16 MB buffer per call)

    def fasta(self, read_ids, with_ends: bool = False, as_array: bool = False, out_alloc=None):
        """FASTA records of every target of the job, target order (herro_job_fasta: one sizing call, one call that writes the
        text straight into a numpy buffer; the library's thread pool assembles it).  read_ids: one str/bytes per target.
        with_ends: also the end offset of every target's records.  as_array: the text as a u8 array (no bytes copy).
        out_alloc(nbytes) -> u8 array: where the text goes (a reusable buffer: a fresh 16 MB array costs more in page faults than
        the library needs to fill it)."""
        n = len(read_ids)
        if n != self.n_targets:   # the library reads one id and writes one end offset per target of the job
            raise ValueError(f"read_ids has {n} entries, the job has {self.n_targets} targets")
        arr = (C.c_char_p * max(n, 1))(*[r if isinstance(r, bytes) else r.encode() for r in read_ids])
        ends = np.zeros(max(n, 1), np.uint64)
        need = self._l.herro_job_fasta(self.h, arr, None, None, 0, ends.ctypes.data)
        if need < 0:
            self.ctx._chk(int(need))
        out = np.empty(max(int(need), 1), np.uint8) if out_alloc is None else out_alloc(max(int(need), 1))
        got = self._l.herro_job_fasta(self.h, arr, None, out.ctypes.data, int(need), None)
        if got < 0:
            self.ctx._chk(int(got))
        text = out[:got] if as_array else out[:got].tobytes()
        return (text, ends[:n]) if with_ends else text

    def fasta_dev(self, read_ids, descs=None, chop_len: int = 0, min_length: int = 0, line_width: int = 0, with_ends: bool = False,
                  as_array: bool = False, with_stats: bool = False):
        """FASTA records of every target of the job, formed on the device (herro_job_fasta_dev): with the three numbers 0 the
        text of fasta(), byte for byte; chop_len C > 0 cuts every record into pieces of C bases named <name>_sliding:<start>-<end> (seqkit sliding
        -s C -W C -g), min_length drops the pieces below it (seqkit seq -m), line_width wraps the bodies — **POSTPROCESS is what
        scripts/postprocess_corrected.sh runs before the assembler.  read_ids: one str / bytes per target, None: the target gives nothing; descs:
        None, or one str / bytes / None per target.  with_ends: also the end offset of every target's records; with_stats: also a FastaStats;
        as_array: the text as a u8 array over the library's buffer (no copy; the buffer is freed with the array)."""
        n = len(read_ids)
        if n != self.n_targets:
            raise ValueError(f"read_ids has {n} entries, the job has {self.n_targets} targets")
        if descs is not None and len(descs) != n:
            raise ValueError(f"descs has {len(descs)} entries, the job has {n} targets")
        ids = (C.c_char_p * max(n, 1))(*[_c_str(r) for r in read_ids])
        ds = None if descs is None else (C.c_char_p * max(n, 1))(*[_c_str(d) for d in descs])
        p = _chop_params(chop_len, min_length, line_width)
        h = C.c_void_p()
        L = self._l
        self.ctx._chk(L.herro_job_fasta_dev(self.h, ids, ds, C.byref(p), C.byref(h)))
        try:
            nb = int(L.herro_fasta_text_len(h))
            ends = np.zeros(n, np.uint64)
            if n:
                C.memmove(ends.ctypes.data, L.herro_fasta_text_target_end(h), ends.nbytes)
            st = (C.c_uint64 * 6)()
            L.herro_fasta_text_stats(h, st)
            if as_array and nb:
                buf = (C.c_uint8 * nb).from_address(L.herro_fasta_text_data(h))
                weakref.finalize(buf, L.herro_fasta_text_free, h)   # the array's base keeps buf alive; the handle goes with it
                h = None
                text = np.frombuffer(buf, np.uint8)
            elif as_array:
                text = np.zeros(0, np.uint8)
            else:
                text = C.string_at(L.herro_fasta_text_data(h), nb) if nb else b""
        finally:
            if h is not None:
                L.herro_fasta_text_free(h)
        out = (text,) + ((ends,) if with_ends else ()) + ((FastaStats(*[int(x) for x in st]),) if with_stats else ())
        return out[0] if len(out) == 1 else out

    def rf_left(self) -> int:
        """test hook: windows of the last infer whose receptive fields k_rfq filled BEHIND a fused gather (more informative rows than k_rows stages)"""
        rc = self._l.herro_debug_job_rf_left(self.h)
        if rc < 0:
            self.ctx._chk(rc)
        return rc

    def rf_fused(self) -> bool:
        """test hook: the last infer read the receptive fields k_rows gathered itself (False: k_rfq's)"""
        rc = self._l.herro_debug_job_rf_fused(self.h)
        if rc < 0:
            self.ctx._chk(rc)
        return rc == 1

    def rf_records(self, w: int) -> np.ndarray:
        """test hook: the receptive-field records the model read for window w, [n_supported, 31, 16] (bytes 0..7 tokens, 8..15 qualities)"""
        ns = self.info(w).n_supported
        out = np.zeros((ns, 31, 16), np.uint8)
        n = self._l.herro_debug_job_rf(self.h, w, out.ctypes.data, out.nbytes)
        if n < 0:
            self.ctx._chk(int(n))
        assert n == ns * 31
        return out

    def directory_words(self, ow: int, nw: int) -> np.ndarray:
        """test hook: the directory words k_cols wrote for overlap-window `ow` (herro_debug_job_cwd), u32 [nw = ceil(window size / 32)]"""
        out = np.zeros(nw, np.uint32)
        n = self._l.herro_debug_job_cwd(self.h, ow, out.ctypes.data, nw)
        if n < 0:
            self.ctx._chk(int(n))
        assert n == nw, (n, nw)
        return out

    def set_base_logits(self, base: np.ndarray):
        """test hook: base logits [informative rows of the job, 5] (job order) replace the model's; the consensus is dropped
        (herro_debug_job_set_base_logits)"""
        b = np.ascontiguousarray(base, np.float32)
        assert b.ndim == 2 and b.shape[1] == 5, b.shape
        self.ctx._chk(self._l.herro_debug_job_set_base_logits(self.h, b.ctypes.data, b.shape[0]))

    def stats(self) -> dict[str, int]:
        o = np.zeros(6, np.uint64)
        self.ctx._chk(self._l.herro_job_stats(self.h, o.ctypes.data))
        k = ("read_bytes", "op_bytes", "out_bytes", "sum_len", "sum_supported", "n_model_windows")
        return {a: int(b) for a, b in zip(k, o)}


def _name_blob(ctx: "Context", names: list[bytes]):
    """(names back to back, name_off u64 [n_reads + 1]) as the PAF writer and herro_name_index_create take them"""
    if len(names) != getattr(ctx, "n_reads", len(names)):
        raise ValueError(f"{len(names)} names for {ctx.n_reads} reads")
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(n) for n in names])
    return b"".join(names), off


def _paf_text_bytes(L, h) -> bytes:
    try:
        n = int(L.herro_paf_text_len(h))
        return C.string_at(L.herro_paf_text_data(h), n) if n else b""
    finally:
        L.herro_paf_text_free(h)


class AlignedDev:
    """herro_aligned_dev: aligned records whose ops live on the device.  rows u32 [n, 10] (trimmed coordinates, cigar_len 0),
    scores i32 [n], n_ops u32 [n], ok bool [n] (False: failed, no ops)."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h, self._l = ctx, h, ctx._l
        n = self.n = int(self._l.herro_aligned_dev_n(h))
        self.rows = _aln_rows(self._l.herro_aligned_dev_alignments(h), n)
        self.scores = np.zeros(n, np.int32)
        self.n_ops = np.zeros(n, np.uint32)
        if n:
            self.scores[:] = np.ctypeslib.as_array(C.cast(self._l.herro_aligned_dev_scores(h), C.POINTER(C.c_int32)), (n,))
            self.n_ops[:] = np.ctypeslib.as_array(C.cast(self._l.herro_aligned_dev_n_ops(h), C.POINTER(C.c_uint32)), (n,))
        self.ok = self.n_ops > 0
        self.failed = int(self._l.herro_aligned_dev_failed(h))

    def cigar(self, r: int) -> bytes:
        """record r's CIGAR text (herro_aligned_dev_cigar: its ops come down and are formatted for this call); b"" for a failed record"""
        cap = 11 * int(self.n_ops[r]) + 1 if 0 <= r < self.n else 1
        buf = C.create_string_buffer(cap)
        n = self._l.herro_aligned_dev_cigar(self.h, r, buf, cap)
        if n < 0:
            raise HerroError(int(n), "herro_aligned_dev_cigar")
        return C.string_at(buf, n)

    def paf(self, names: list[bytes], rec=None) -> bytes:
        """herro_aligned_dev_paf: the PAF lines (with cg:Z:) of records rec, in that order (None: all of them) — formed on the device for a
        device handle, by the host formatter for a HostContext's; failed records give no line.  names: the read names, index = read id."""
        blob, off = _name_blob(self.ctx, names)
        if rec is None:
            n_rows, rp = self.n, None
        else:
            rec = np.ascontiguousarray(rec, np.uint32)
            n_rows = len(rec)
            buf = rec if n_rows else np.zeros(1, np.uint32)   # (never a NULL pointer: that would mean "row i is record i")
            rp = buf.ctypes.data
        h = C.c_void_p()
        self.ctx._chk(self._l.herro_aligned_dev_paf(self.ctx.h, self.h, n_rows, rp, blob, off.ctypes.data, C.byref(h)))
        return _paf_text_bytes(self._l, h)

    def mirror(self) -> "AlignedDev":
        """herro_aligned_dev_mirror: a new handle of 2n records — record r is this handle's record r, record n + r its mirror, the
        alignment with query and target exchanged, derived from the ops on the device instead of aligned again (pair_rows and
        paired_job_args do the bookkeeping).  This handle may be closed afterwards."""
        h = C.c_void_p()
        self.ctx._chk(self._l.herro_aligned_dev_mirror(self.ctx.h, self.h, C.byref(h)))
        return AlignedDev(self.ctx, h)

    def close(self):
        if getattr(self, "h", None):
            self._l.herro_aligned_dev_free(self.h)
            self.h = None

    __del__ = close


class OverlapPairs:
    """herro_pairs: one record per overlapping read pair and the table of the finder's two rows per pair.  n_pairs = P; primaries u32
    [P, 10] (ascending (tid, qid), extended unless extend=False, cigar_len 0); chain_scores i32 [P]; ext u32 [P, 4] and ext_scores i32
    [P, 2] as extend_overlaps returns them (zeros without extension or from a table); rids u32 [n_targets], aln_off u64 [n_targets + 1],
    rec_of_row u32 [n_rows] as find_overlaps and pair_rows give them; n_rows = 2 P, fewer for a handle of core targets (find_overlap_pairs(core=...):
    the rows whose target is core); occ_cut: the frequency cut the finder used (0 for a handle over a table)."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h, self._l = ctx, h, ctx._l
        L = self._l
        n = self.n_pairs = int(L.herro_pairs_n(h))
        nt = int(L.herro_pairs_n_targets(h))
        self.n_rows = int(L.herro_pairs_n_rows(h)) if hasattr(L, "herro_pairs_n_rows") else 2 * n
        self.occ_cut = int(L.herro_pairs_occ_cut(h)) if hasattr(L, "herro_pairs_occ_cut") else 0
        self.rescued = int(L.herro_pairs_rescued(h)) if hasattr(L, "herro_pairs_rescued") else 0   # minimizers the rescue kept (0: off)
        self.index_blocks = int(L.herro_pairs_index_blocks(h)) if hasattr(L, "herro_pairs_index_blocks") else 0   # read blocks of an index in parts (0: off)

        def arr(ptr, ct, dt, shape):
            out = np.zeros(shape, dt)
            if out.size:
                out[...] = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape)
            return out
        self.primaries = _aln_rows(L.herro_pairs_primaries(h), n)
        self.chain_scores = arr(L.herro_pairs_chain_scores(h), C.c_int32, np.int32, (n,))
        self.ext = arr(L.herro_pairs_ext(h), C.c_uint32, np.uint32, (n, 4))
        self.ext_scores = arr(L.herro_pairs_ext_scores(h), C.c_int32, np.int32, (n, 2))
        self.rids = arr(L.herro_pairs_target_ids(h), C.c_uint32, np.uint32, (nt,))
        self.aln_off = arr(L.herro_pairs_aln_off(h), C.c_uint64, np.uint64, (nt + 1,))
        self.rec_of_row = arr(L.herro_pairs_rec_of_row(h), C.c_uint32, np.uint32, (self.n_rows,))

    def align(self) -> "AlignedDev":
        """herro_pairs_align: Context.align_dev(self.primaries).mirror() — 2 P records, primaries then mirrors."""
        h = C.c_void_p()
        self.ctx._chk(self._l.herro_pairs_align(self.ctx.h, self.h, C.byref(h)))
        return AlignedDev(self.ctx, h)

    def paf(self, m: "AlignedDev", names: list[bytes]) -> bytes:
        """herro_pairs_paf: the PAF lines of the table's rows, in its order, from the handle align() returned — the alignments
        Context.create_job_paired builds its job from (rows whose record failed give no line)."""
        blob, off = _name_blob(self.ctx, names)
        h = C.c_void_p()
        self.ctx._chk(self._l.herro_pairs_paf(self.ctx.h, self.h, m.h, blob, off.ctypes.data, C.byref(h)))
        return _paf_text_bytes(self._l, h)

    def write_alns(self, m: "AlignedDev", names: list[bytes], path: str, oec: bool | None = None) -> tuple[int, int]:
        """herro_pairs_write_alns: the lines of paf() streamed to `path` — as the reference's batch file (one zstd frame: target count, target
        names, lines; what `--write-alns` writes and `--read-alns` / Paf(path=...) read) when oec, which None decides by the suffix
        .oec.zst; plain PAF otherwise.  Returns (lines, bytes of the file)."""
        blob, off = _name_blob(self.ctx, names)
        if oec is None:
            oec = str(path).endswith(".oec.zst")
        lines, size = C.c_uint64(), C.c_uint64()
        self.ctx._chk(self._l.herro_pairs_write_alns(self.ctx.h, self.h, m.h, blob, off.ctypes.data, os.fsencode(path), ALNS_OEC if oec else 0,
                                                     C.byref(lines), C.byref(size)))
        return int(lines.value), int(size.value)

    def cluster(self, n_parts: int, weights=None, min_span: int = 0) -> "Clusters":
        """herro_pairs_cluster: the reads of the store partitioned by this handle's primaries — edge (tid, qid) with span min(tend - tstart,
        qend - qstart) as the handle holds them; weights u32 [n_reads] (windows per read, say) or None.  The result does not need this handle."""
        w = None if weights is None else np.ascontiguousarray(weights, np.uint32).reshape(-1)
        if w is not None and len(w) != self.ctx.n_reads:
            raise ValueError("weights has one entry per read of the store")
        if not 0 <= int(n_parts) <= 0xFFFFFFFF or not 0 <= int(min_span) <= 0xFFFFFFFF:
            raise HerroError(-1, "cluster parameters: n_parts and min_span are unsigned 32-bit values")
        P = ClusterParams(n_parts=int(n_parts), min_span=int(min_span))
        h = C.c_void_p()
        self.ctx._chk(self._l.herro_pairs_cluster(self.ctx.h, self.h, None if w is None else w.ctypes.data, C.byref(P), C.byref(h)))
        return Clusters(self.ctx, h)

    def close(self):
        if getattr(self, "h", None):
            self._l.herro_pairs_free(self.h)
            self.h = None

    __del__ = close


CLUSTER_STATS = ("n_components", "n_levels", "strong_edges", "edge_cut")
CLUSTER_PART_STATS = ("n_core", "weight", "n_neighbours", "pairs_inside", "pairs_touching")


class Clusters:
    """herro_clusters: the reads partitioned by their overlap graph (Context.cluster_graph, OverlapPairs.cluster) — what the reference's
    workflow gets from scripts/create_clusters.py.  n_parts, n_reads; part, rank, comp, level u32 [n_reads]; stats: dict of CLUSTER_STATS;
    part_stats u64 [n_parts, 5] in the order of CLUSTER_PART_STATS.  mask(p): u8 [n_reads], 1 core, 2 neighbour, 0 neither, made on the device
    from the graph the handle keeps there; as a `core` argument of find_overlap_pairs pass mask(p) == 1."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h, self._l = ctx, h, ctx._l
        L = self._l
        k = self.n_parts = int(L.herro_clusters_n_parts(h))
        n = self.n_reads = int(L.herro_clusters_n_reads(h))

        def arr(ptr):
            out = np.zeros(n, np.uint32)
            if n:
                C.memmove(out.ctypes.data, ptr, out.nbytes)
            return out
        self.part, self.rank = arr(L.herro_clusters_part(h)), arr(L.herro_clusters_rank(h))
        self.comp, self.level = arr(L.herro_clusters_comp(h)), arr(L.herro_clusters_level(h))
        g = np.zeros(4, np.uint64)
        ctx._chk(L.herro_clusters_stats(h, g.ctypes.data))
        self.stats = {name: int(v) for name, v in zip(CLUSTER_STATS, g)}
        self.part_stats = np.zeros((k, 5), np.uint64)
        for p in range(k):
            ctx._chk(L.herro_clusters_part_stats(h, p, self.part_stats[p].ctypes.data))

    def mask(self, p: int) -> np.ndarray:
        out = np.zeros(max(self.n_reads, 1), np.uint8)
        self.ctx._chk(self._l.herro_clusters_mask(self.h, int(p), out.ctypes.data))
        return out[:self.n_reads]

    def core_masks(self) -> list[np.ndarray]:
        """one core mask per part in the shape shard.core_masks returns (u8 [n_reads], 1 = the read is the part's target): from `part`, no device call"""
        return [(self.part == p).astype(np.uint8) for p in range(self.n_parts)]

    def close(self):
        if getattr(self, "h", None):
            self._l.herro_clusters_free(self.h)
            self.h = None

    __del__ = close


OW_DTYPE = np.dtype([(n, "<u4") for n in ("win", "qid", "cls", "tstart", "qbeg", "qlen", "op_begin", "op_cnt", "start_off",
                                            "end_off", "scr_off", "strand", "wtstart", "wlen")] +
                    [(n, "<u8") for n in ("t_woff", "q_woff", "q_qual_off")], align=True)   # OwDesc (csrc/pileup_core.h)
WIN_DTYPE = np.dtype([(n, "<u4") for n in ("rid", "wid", "n_wids", "tstart", "win_len", "ow_begin", "ow_cnt", "lub")] +
                     [(n, "<u8") for n in ("col_off", "fin_off", "row_off", "pos_off", "ev_off")], align=True)   # WinDesc


class HostContext(Context):
    """Device-free context for testing the host half of herro_job_create (herro_debug_host_ctx)."""

    def __init__(self, read_len, name_class=None):
        self._l = lib()
        rl = np.ascontiguousarray(read_len, np.uint32)
        nc = None if name_class is None else np.ascontiguousarray(name_class, np.uint32)
        self.h = self._l.herro_debug_host_ctx(len(rl), rl.ctypes.data, None if nc is None else nc.ctypes.data)
        self.n_reads = len(rl)

class NameIndex:
    """read name -> read id, built once per read set (herro_name_index_create; the reference's `name_to_id`, lib.rs:136-140)."""

    def __init__(self, names: list[bytes]):
        self.h = None
        L = lib()
        blob = b"".join(names)
        off = np.zeros(len(names) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in names])
        self._l, self.n = L, len(names)
        self.h = L.herro_name_index_create(len(names), blob, off.ctypes.data)
        if not self.h:
            raise HerroError(-1, "herro_name_index_create")

    def close(self):
        if self.h:
            self._l.herro_name_index_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Paf:
    """Parsed PAF / .oec.zst batch (host only; overlaps.rs:117-202, 292-323): targets in order of first
    appearance, their alignments in file order.  `targets`, `aln_off`, `alns` are what herro_job_create takes;
    the CIGAR pointers inside `alns` stay valid while this object lives.  `names`: the read ids, or a NameIndex built once."""

    def __init__(self, names, text: bytes | None = None, path: str | None = None, core=None, threads: int = 0, view: bool = False,
                 cigars: bool = True):
        """view=True (with a NameIndex and `text`): no copy of the text — this object keeps `text` alive instead.
        cigars=False: a PAF without CIGARs (herro_paf_parse_coords; `text` only) — records for Context.align, cigar_len 0."""
        self.h = None
        self._text = text if view else None
        L = lib()
        core_a = None if core is None else np.ascontiguousarray(core, np.uint8)
        err = C.create_string_buffer(512)
        cptr = None if core_a is None else core_a.ctypes.data
        if not cigars:
            if text is None:
                raise ValueError("Paf(cigars=False) parses PAF text only")
            ix = names if isinstance(names, NameIndex) else NameIndex(names)
            try:
                h = L.herro_paf_parse_coords(text, len(text), ix.h, cptr, threads, err, 512)
            finally:
                if ix is not names:
                    ix.close()
        elif isinstance(names, NameIndex):
            if text is not None and view:
                h = L.herro_paf_parse_view(text, len(text), names.h, cptr, threads, err, 512)
            elif text is not None:
                h = L.herro_paf_parse_indexed(text, len(text), names.h, cptr, threads, err, 512)
            else:
                h = L.herro_oec_read_indexed(path.encode(), names.h, cptr, threads, err, 512)
        else:
            blob = b"".join(names)
            off = np.zeros(len(names) + 1, np.uint64)
            off[1:] = np.cumsum([len(n) for n in names])
            if text is not None:
                h = L.herro_paf_parse(text, len(text), len(names), blob, off.ctypes.data, cptr, threads, err, 512)
            else:
                h = L.herro_oec_read(path.encode(), len(names), blob, off.ctypes.data, cptr, threads, err, 512)
        if not h:
            raise HerroError(-3, err.value.decode())
        self._l, self.h = L, h
        n = L.herro_paf_n_targets(h)
        self.targets = np.ctypeslib.as_array(C.cast(L.herro_paf_target_ids(h), C.POINTER(C.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)
        self.aln_off = np.ctypeslib.as_array(C.cast(L.herro_paf_aln_off(h), C.POINTER(C.c_uint64)), (n + 1,)).copy()
        na = int(self.aln_off[-1])
        self.n_alns = na
        self._alns_ptr = L.herro_paf_alignments(h)
        self.alns = (Alignment * na).from_address(self._alns_ptr) if na else []

    def coords(self) -> np.ndarray:
        """u32 [n, 10]: qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend, cigar_len in output order (Context.align's rows)."""
        return _aln_rows(self._alns_ptr, self.n_alns)

    def rows(self):
        """[(qid, qlen, qstart, qend, strand, tid, tlen, tstart, tend, cigar bytes)] in output order."""
        out = []
        for a in self.alns:
            out.append((a.qid, a.qlen, a.qstart, a.qend, a.strand, a.tid, a.tlen, a.tstart, a.tend,
                        C.string_at(a.cigar, a.cigar_len) if a.cigar_len else b""))
        return out

    def close(self):
        if self.h:
            self._l.herro_paf_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class PreparedAlignments:
    """All alignments of a data set as ONE herro_alignment array, grouped by target — what a host holds after parsing its
    PAF / .oec.zst input (the reference's reader thread hands `(tid, Vec<Alignment>)` to the feature threads,
    lib.rs:141-151).  Jobs over target ranges are then pure C calls: no per-job packing on the Python side."""

    def __init__(self, sb):
        n = len(sb.aln)
        self.rids = np.ascontiguousarray(sb.tgt_rid, np.uint32)
        self.aln_off = np.ascontiguousarray(sb.tgt_aln_off, np.uint64)
        self._cig = np.ascontiguousarray(sb.cig, np.uint8)
        self._arr, view = _aln_array(sb.aln, 10)
        if n:
            view["p"][:n] = self._cig.ctypes.data + np.asarray(sb.cig_off, np.uint64)
        self.n_targets = len(self.rids)
        self._reg = None

    def register(self, ctx: "Context"):
        """pin the CIGAR blob for zero-copy job creation (herro_host_register); undo with unregister() before the arrays go away"""
        if self._reg is None and len(self._cig):
            try:
                ctx.register_host(self._cig)
            except HerroError as e:       # e.g. the memlock limit: jobs are staged instead (the zero-copy path is an optimisation, never a requirement)
                if e.code != -4:   # HERRO_E_UNSUPPORTED
                    raise
                return
            self._reg = True

    def unregister(self):
        if self._reg is not None:
            rc = lib().herro_host_unregister(None, self._cig.ctypes.data)   # the registry is process-wide: no context needed (the one that registered may be closed by now)
            if rc:
                raise HerroError(int(rc), "herro_host_unregister")
            self._reg = None

    def job(self, ctx: "Context", t0: int, t1: int, window_size: int) -> "Job":
        """herro_job_create over targets [t0, t1): rids / aln_off are passed as offsets into the resident arrays"""
        h = ctx._l.herro_job_create(ctx.h, t1 - t0, self.rids.ctypes.data + 4 * t0, self.aln_off.ctypes.data + 8 * t0,
                                    C.byref(self._arr), window_size)
        return _job_or_raise(ctx, h, t1 - t0)


def job_from_synth(ctx: Context, sb, window_size: int, targets=None) -> Job:
    """Job over targets of a SynthBatch (all by default)."""
    ts = list(range(sb.n_targets)) if targets is None else list(targets)
    a0 = [int(sb.tgt_aln_off[t]) for t in ts]
    a1 = [int(sb.tgt_aln_off[t + 1]) for t in ts]
    sel = np.concatenate([np.arange(x, y) for x, y in zip(a0, a1)]).astype(np.int64) if ts else np.zeros(0, np.int64)
    off = np.zeros(len(ts) + 1, np.uint64)
    off[1:] = np.cumsum([y - x for x, y in zip(a0, a1)])
    rows = sb.aln[sel]
    return ctx.create_job(sb.tgt_rid[ts], rows, off, None, window_size, cig_blob=sb.cig, cig_off=sb.cig_off[sel])


def aligned_job_args(rids, aln_off, rows_out: np.ndarray, cigars: list[bytes], ok: np.ndarray):
    """The AlnMode::None counterpart of parse_paf's output (overlaps.rs:340-344): drops the records Context.align failed, regroups
    aln_off over the targets and returns (rids, rows, aln_off, cigars) for Context.create_job.  Targets keep their place even when
    all their records failed."""
    rids = np.ascontiguousarray(rids, np.uint32)
    aln_off = np.asarray(aln_off, np.int64)
    ok = np.asarray(ok, bool)
    kept = np.concatenate([[0], np.cumsum(ok)]).astype(np.int64)
    return rids, np.ascontiguousarray(rows_out[ok]), kept[aln_off].astype(np.uint64), [c for c, k in zip(cigars, ok) if k]


def aligned_dev_job_args(rids, aln_off, ok: np.ndarray):
    """aligned_job_args for Context.create_job_aligned: (rids, aln_off', rec) with the failed records (ok False) dropped — rec holds the
    indices of the kept ones in the handle, aln_off' regroups them over the targets.  Targets keep their place even when all their
    records failed."""
    rids = np.ascontiguousarray(rids, np.uint32)
    aln_off = np.asarray(aln_off, np.int64)
    ok = np.asarray(ok, bool)
    kept = np.concatenate([[0], np.cumsum(ok)]).astype(np.int64)
    return rids, kept[aln_off].astype(np.uint64), np.flatnonzero(ok).astype(np.uint32)


FastaStats = collections.namedtuple("FastaStats", "records bases pieces_dropped bases_dropped segments targets")
ChopStats = collections.namedtuple("ChopStats", "pieces_kept pieces_dropped bases_kept bases_dropped")


def _c_str(x):
    return x if x is None or isinstance(x, bytes) else x.encode()


def _chop_params(chop_len, min_length, line_width) -> ChopParams:
    vals = dict(chop_len=int(chop_len), min_length=int(min_length), line_width=int(line_width))
    for name, v in vals.items():
        if not 0 <= v <= 0xFFFFFFFF:
            raise ValueError(f"{name} = {v}: a 32-bit unsigned number")
    return ChopParams(**vals)


def chop_plan(lengths, chop_len: int = 0, min_length: int = 0, line_width: int = 0):
    """The pieces Job.fasta_dev keeps of sequences of these lengths (herro_chop_plan; host code, no device): pieces of chop_len bases, the last
    one of a sequence shorter, those below min_length dropped; chop_len 0: the sequence is its one piece.  Returns (pieces PIECE_DTYPE — rid is
    the sequence — grouped by sequence, piece_off u64 [n + 1], ChopStats); ValueError with the library's message on a refusal."""
    ln = np.ascontiguousarray(lengths, np.uint64)
    return _chop_plan(lib(), ln, _chop_params(chop_len, min_length, line_width))


def index_plan(lens, k: int = 25, w: int = 17, max_kmers: int = 0, ctx: "Context | None" = None) -> np.ndarray:
    """The read blocks of an index in parts (herro_index_plan; host code, no device): cuts u64 [n_blocks + 1], ascending read ids from 0 to
    len(lens) — block b is the reads cuts[b] .. cuts[b + 1] - 1; an empty store has no block.  The rule is include/herro_amd.h's, "an index in
    parts".  ctx: the context to ask (a HostContext does); None: a device-free one made for the call."""
    ln = np.ascontiguousarray(lens, np.uint32).reshape(-1)
    own = ctx is None
    if own:
        ctx = HostContext(ln[:1] if len(ln) else np.ones(1, np.uint32))
    try:
        n = ctx._l.herro_index_plan(ctx.h, len(ln), ln.ctypes.data if len(ln) else None, int(k), int(w), int(max_kmers), None, 0)
        if n < 0:
            ctx._chk(int(n))
        cuts = np.zeros(n + 1, np.uint64)
        got = ctx._l.herro_index_plan(ctx.h, len(ln), ln.ctypes.data if len(ln) else None, int(k), int(w), int(max_kmers), cuts.ctypes.data, len(cuts))
        assert got == n
    finally:
        if own:
            ctx.close()
    return cuts


def _chop_plan(L, ln, p):
    h, err = C.c_void_p(), C.create_string_buffer(256)
    rc = L.herro_chop_plan(len(ln), ln.ctypes.data if ln is not None else None, C.byref(p) if p is not None else None, C.byref(h), err, 256)
    if rc:
        raise ValueError(err.value.decode())
    try:
        n = int(L.herro_trim_n_pieces(h))
        pieces = np.zeros(n, PIECE_DTYPE)
        if n:
            C.memmove(pieces.ctypes.data, L.herro_trim_pieces(h), pieces.nbytes)
        piece_off = np.zeros(len(ln) + 1, np.uint64)
        C.memmove(piece_off.ctypes.data, L.herro_trim_piece_off(h), piece_off.nbytes)
        st = (C.c_uint64 * 4)()
        L.herro_trim_stats(h, st)
    finally:
        L.herro_trim_free(h)
    return pieces, piece_off, ChopStats(*[int(x) for x in st])


TrimStats = collections.namedtuple("TrimStats", "reads_trimmed reads_split reads_dropped bases_removed")


def trim_plan(read_len, adapter_len, hits, hits_off, end_window: int = 0, end_max_err_pm: int = 0, mid_max_err_pm: int = 0, min_length: int = 0,
              discard_chimeras: bool = False):
    """The pieces of every read that stay, from find_adapters' hits (herro_trim_plan; host code, no device): adapters at the read ends are trimmed,
    a read is split at an adapter in its middle (discard_chimeras: dropped), pieces shorter than min_length are dropped.  0 = the default:
    end_window 150, end_max_err_pm 250, mid_max_err_pm 100.  read_len u32 [n_reads], adapter_len u32 [n_adapters].
    Returns (pieces PIECE_DTYPE grouped by read, piece_off u64 [n_reads + 1], TrimStats); ValueError with the library's message on a bad table."""
    L = lib()
    rl = np.ascontiguousarray(read_len, np.uint32)
    al = np.ascontiguousarray(adapter_len, np.uint32)
    hits = np.ascontiguousarray(hits, ADAPTER_HIT_DTYPE)
    ho = np.ascontiguousarray(hits_off, np.uint64)
    if len(ho) != len(rl) + 1:
        raise ValueError("herro_trim_plan: hits_off has n_reads + 1 entries")
    if len(ho) and int(ho.max()) > len(hits):
        raise ValueError("herro_trim_plan: hits_off reaches beyond the hits")
    p = TrimParams(end_window=int(end_window), end_max_err_pm=int(end_max_err_pm), mid_max_err_pm=int(mid_max_err_pm), min_length=int(min_length),
                   flags=TRIM_DISCARD_CHIMERAS if discard_chimeras else 0)
    return _trim_plan(L, rl, al, hits, ho, p)


def _trim_plan(L, rl, al, hits, ho, p):
    h, err = C.c_void_p(), C.create_string_buffer(256)
    rc = L.herro_trim_plan(len(rl), rl.ctypes.data, len(al), al.ctypes.data, hits.ctypes.data, ho.ctypes.data, C.byref(p), C.byref(h), err, 256)
    if rc:
        raise ValueError(err.value.decode())
    try:
        n = int(L.herro_trim_n_pieces(h))
        pieces = np.zeros(n, PIECE_DTYPE)
        if n:
            C.memmove(pieces.ctypes.data, L.herro_trim_pieces(h), pieces.nbytes)
        piece_off = np.zeros(len(rl) + 1, np.uint64)
        C.memmove(piece_off.ctypes.data, L.herro_trim_piece_off(h), piece_off.nbytes)
        st = (C.c_uint64 * 4)()
        L.herro_trim_stats(h, st)
    finally:
        L.herro_trim_free(h)
    return pieces, piece_off, TrimStats(*[int(x) for x in st])


def trim_reads(ctx: "Context", reads, adapters, max_err_pm: int = 0, forward_only: bool = False, on_device: bool = False, **plan_params):
    """Raw reads to a trimmed store in one call: set_reads(reads), find_adapters, trim_plan, io.cut_reads, set_reads(the cut reads).  reads: an
    io.Reads; adapters, max_err_pm, forward_only as find_adapters; plan_params as trim_plan.  Returns (the cut io.Reads — what the store now
    holds —, TrimStats).
    on_device: the last two steps are Context.cut_store — the store is cut where it lies and no base is copied on the host.  The io.Reads that
    comes back then has the cut reads' ids, descriptions and offsets (io.cut_names) and seq = qual = None: the bases are in the store."""
    from . import io
    ctx.set_reads(reads.seq, reads.qual, reads.off)
    hits, hits_off = ctx.find_adapters(adapters, max_err_pm=max_err_pm, forward_only=forward_only)
    pieces, _, stats = trim_plan(np.diff(np.asarray(reads.off, np.uint64)).astype(np.uint32), [len(a) for a in adapters], hits, hits_off, **plan_params)
    if on_device:
        ids, descs, off = io.cut_names(reads.ids, reads.descriptions, reads.off, pieces)
        ctx.cut_store(pieces)
        return io.Reads(ids, descs, None, None, off), stats
    cut = io.cut_reads(reads, pieces)
    ctx.set_reads(cut.seq, cut.qual, cut.off)
    return cut, stats


def pair_rows(rows: np.ndarray, exact_ids: bool = False):
    """Pairs the two directions of an overlap, so that one of them is aligned and the other mirrored (AlignedDev.mirror).  Row j is
    the mate of row i iff it is exactly i's swap — query and target fields exchanged, the same strand — which is what find_overlaps
    emits for a pair; a row whose other direction differs in any coordinate has no mate and is aligned itself.  Returns (prim,
    rec_of_row): prim i64 — the first row of every pair and every row without a mate, in row order; rec_of_row u32 [n] — the record
    that a mirrored handle over rows[prim] holds for row i: p for prim[p] == i, len(prim) + p for the mate of prim[p].  To be called
    before extend_overlaps: independently extended directions are no longer exact swaps.  exact_ids: class the rows by np.unique
    instead of by the checked hash (what a hash collision falls back to; for tests)."""
    rows = np.ascontiguousarray(np.asarray(rows)[:, :9], np.uint32)
    n = len(rows)
    swapped = np.ascontiguousarray(rows[:, [5, 6, 7, 8, 4, 0, 1, 2, 3]])
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint32)
    # The two directions of an overlap share a canonical row: the smaller of the row and its swap.  `side` says which of the two a
    # row is; a row equal to its own swap has side 0 and a class of its own kind.
    differ = rows != swapped
    col = differ.argmax(axis=1)
    at = np.arange(n)
    side = rows[at, col] > swapped[at, col]
    own = ~differ.any(axis=1)
    canon = np.where(side[:, None], swapped, rows)
    # classes by a 64-bit hash of the canonical row, checked: rows that sort together must be equal, else the exact ids are taken
    mult = np.array([0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93, 0xFF51AFD7ED558CCD,
                     0xC4CEB9FE1A85EC53, 0x2545F4914F6CDD1D, 0x94D049BB133111EB, 0xBF58476D1CE4E5B9], np.uint64)
    with np.errstate(over="ignore"):
        key = (canon.astype(np.uint64) * mult).sum(axis=1, dtype=np.uint64)
        key ^= key >> np.uint64(29)
    for exact in ((True,) if exact_ids else (False, True)):
        if exact:
            key = np.unique(canon.view(np.dtype((np.void, 36))).ravel(), return_inverse=True)[1].astype(np.uint64)
        o = np.lexsort((side, key))                                       # by class, then side; stable: row order within
        first = np.ones(n, bool)
        first[1:] = key[o][1:] != key[o][:-1]
        if exact or not (canon[o][1:][~first[1:]] != canon[o][:-1][~first[1:]]).any():
            break
    # Within a class the k-th row of one side pairs with the k-th row of the other — what taking the rows in order and giving each
    # the oldest unpaired row of the other direction comes to; rows equal to their own swap pair up two by two.
    start = np.maximum.accumulate(np.where(first, at, 0))
    cls = np.cumsum(first) - 1
    n_a = np.add.reduceat((~side[o]).astype(np.int64), np.flatnonzero(first))[cls]      # rows of side 0 in the class
    k = at - start
    second = np.where(own[o], (k & 1) == 1, side[o] & (k - n_a < n_a))   # (sorted position) a row that pairs with an earlier-sorted one
    partner = np.where(own[o], at - 1, start + k - n_a)
    x, y = o[second], o[partner[second]]
    head, mate = np.minimum(x, y), np.maximum(x, y)
    is_prim = np.ones(n, bool)
    is_prim[mate] = False
    prim = np.flatnonzero(is_prim).astype(np.int64)
    rec = np.cumsum(is_prim) - 1
    rec[mate] = len(prim) + rec[head]
    return prim, rec.astype(np.uint32)


def paired_job_args(rids, aln_off, rec_of_row, ok: np.ndarray):
    """aligned_dev_job_args for a mirrored handle: (rids, aln_off', rec) for Context.create_job_aligned, where `ok` is the mirrored
    handle's (2 len(prim) records) and rec_of_row is pair_rows'.  Rows whose record failed are dropped, aln_off' regroups the rest
    over the targets (which keep their place), rec holds their handle indices in row order."""
    rids = np.ascontiguousarray(rids, np.uint32)
    aln_off = np.asarray(aln_off, np.int64)
    rec_of_row = np.asarray(rec_of_row, np.int64)
    keep = np.asarray(ok, bool)[rec_of_row] if len(rec_of_row) else np.zeros(0, bool)
    kept = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return rids, kept[aln_off].astype(np.uint64), rec_of_row[keep].astype(np.uint32)
