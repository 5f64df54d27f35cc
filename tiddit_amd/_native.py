"""ctypes binding of libtiddit_hip.so (include/tiddit_hip.h).  No CPU fallback: a missing library
or a missing GPU raises."""
import ctypes
import os
import sys
import threading


_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("TIDDIT_HIP_LIB") or os.path.join(_HERE, "libtiddit_hip.so")

TDT_OK = 0
ERRORS = {-1: "TDT_E_ARG", -2: "TDT_E_HIP", -3: "TDT_E_RANGE", -4: "TDT_E_INEXACT", -5: "TDT_E_NOMEM",
          -6: "TDT_E_UNSUPPORTED", -7: "TDT_E_KEY"}

_lib = None
_lock = threading.Lock()


class TdtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERRORS.get(code, code), msg))
        self.code = code


# every symbol include/tiddit_hip.h declares: name -> (restype, argtypes)
_i, _i64, _sz, _dbl, _P = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double, ctypes.c_void_p
_PP = ctypes.POINTER(ctypes.c_void_p)
SYMBOLS = {
    "tdt_version": (_i, []),
    "tdt_last_error": (ctypes.c_char_p, []),
    "tdt_build_flags": (ctypes.c_char_p, []),
    "tdt_device_count": (_i, [ctypes.POINTER(_i)]),
    "tdt_ctx_create": (_i, [_i, _PP]),
    "tdt_ctx_destroy": (None, [_P]),
    "tdt_ctx_sync": (_i, [_P]),
    "tdt_ctx_stream": (_P, [_P]),
    "tdt_ctx_set_stream": (_i, [_P, _P]),
    "tdt_ctx_bind_thread": (_i, [_P]),
    "tdt_cov_create": (_i, [_P, _P, _i, _i, _PP]),
    "tdt_cov_destroy": (None, [_P]),
    "tdt_cov_nbins": (_i, [_P, _i, ctypes.POINTER(_i64), ctypes.POINTER(_i)]),
    "tdt_cov_scale_bits": (_i, [_P]),
    "tdt_cov_reset": (_i, [_P]),
    "tdt_cov_push": (_i, [_P, _i, _P, _P, _P, _P, _sz, _i]),
    "tdt_cov_push_device": (_i, [_P, _i, _P, _P, _P, _P, _sz, _i]),
    "tdt_cov_push_device_multi": (_i, [_P, _i, _P, _P, _P, _P, _P, _P, _i]),
    "tdt_cov_pack_device": (_i, [_P, _P, _P, _P, _P, _sz, _P]),
    "tdt_cov_push_packed_device_multi": (_i, [_P, _i, _P, _P, _P, _P, _i]),
    "tdt_cov_pack_binned_device": (_i, [_P, _i, _P, _P, _P, _P, _sz, _P]),
    "tdt_cov_push_binned_device_multi": (_i, [_P, _i, _P, _P, _P, _P, _P, _i]),
    "tdt_cov_total_bins": (_i, [_P, ctypes.POINTER(_i64)]),
    "tdt_cov_offset": (_i, [_P, _i, ctypes.POINTER(_i64)]),
    "tdt_cov_finish_all_device": (_i, [_P, _P]),
    "tdt_cov_finish_all": (_i, [_P, _P]),
    "tdt_cov_finish": (_i, [_P, _i, _P]),
    "tdt_cov_finish_device": (_i, [_P, _i, _P]),
    "tdt_cov_kept": (_i, [_P, ctypes.POINTER(_i64)]),
    "tdt_gc_bins": (_i, [_P, _P, _i64, _i, _dbl, _P]),
    "tdt_gc_bins_fasta": (_i, [_P, _P, _i64, _i64, _i, _i, _i, _dbl, _P]),
    "tdt_gc_bins_fasta_device": (_i, [_P, _P, _i64, _i64, _i, _i, _i, _dbl, _P]),
    "tdt_gc_bins_device": (_i, [_P, _P, _i64, _i, _dbl, _P]),
    "tdt_gc_bins_fasta_many": (_i, [_P, _P, _i64, _i, _P, _P, _P, _P, _P, _i, _dbl, _P, _P, _i64]),
    "tdt_dbscan": (_i, [_P, _P, _sz, _sz, _dbl, _i, _i, _P, ctypes.POINTER(_i64)]),
    "tdt_dbscan_y": (_i, [_P, _P, _sz, _sz, _dbl, _i, _i64, _P, ctypes.POINTER(_i64)]),
    "tdt_dbscan_y_segments": (_i, [_P, _P, _P, _P, _sz, _i, _dbl, _i, _i64, _P, ctypes.POINTER(_i64)]),
    "tdt_dbscan_y_device": (_i, [_P, _P, _P, _sz, ctypes.c_uint64, _i, _i64, _P, _P, ctypes.POINTER(_i)]),
    "tdt_dbscan_device": (_i, [_P, _P, _P, _sz, _P, _i, ctypes.c_uint64, _i, _i, _P, _P]),
    "tdt_sort_dbscan": (_i, [_P, _P, _P, _sz, _P, _i, _dbl, _i, _P, _P]),
    "tdt_sort_dbscan_ex": (_i, [_P, _P, _P, _sz, _P, _i, _dbl, _i, _P, _P, _P, _P]),
    "tdt_cluster_columns": (_i, [_P, _P, _P, _sz, _P, _i, _dbl, _i, _i64, _P, _P, _P]),
    "tdt_host_alloc": (_i, [_sz, _PP]),
    "tdt_host_free": (_i, [_P]),
    "tdt_comm_unique_id": (_i, [_P]),
    "tdt_comm_init": (_i, [_P, _P, _i, _i, _PP]),
    "tdt_comm_destroy": (_i, [_P]),
    "tdt_allgatherv": (_i, [_P, _P, _sz, _P, _P, _P, _i]),
    "tdt_allreduce_sum_f64": (_i, [_P, _P, _sz]),
    "tdt_allgatherv_plan": (_i, [_i, _i, _P, _P, _i, _sz, _P, ctypes.POINTER(_i)]),
    "tdt_signal_select": (_i, [_P, _P, _P, _P, _P, _P, _sz, _P, _i, _i, _i64, _P, ctypes.POINTER(_sz)]),
    "tdt_signal_select_device": (_i, [_P, _P, _P, _P, _P, _P, _sz, _P, _i, _i, _i64, _P, _P]),
    "tdt_signal_scan": (_i, [_P, _P, _sz, _P, _i, _i, _i64, _i, _i, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "tdt_signal_scan_result": (_i, [_P, _P, _P, _P]),
    "tdt_format_clips": (_i, [_P, _P, _P, _P, _sz, ctypes.c_char_p, _P, _sz, ctypes.POINTER(_sz)]),
    "tdt_split_fields": (_i, [_P, _P, _P, _sz, _P, _sz, _i, _P]),
    "tdt_sigtab_create": (_i, [ctypes.c_char_p, _P, _i, _i64, _PP]),
    "tdt_sigtab_destroy": (None, [_P]),
    "tdt_sigtab_add": (_i, [_P, _P, _P, _P, _sz, _sz, _i, _sz, ctypes.POINTER(_sz)]),
    "tdt_sigtab_add_split_row": (_i, [_P, _i, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, _P, _i, _i]),
    "tdt_sigtab_add_clips": (_i, [_P, _i, _P, _sz]),
    "tdt_sigtab_clips": (_i, [_P, _i, _PP, ctypes.POINTER(_sz)]),
    "tdt_sigtab_stats": (_i, [_P, _P]),
    "tdt_sigtab_export": (_i, [_P, _P, _i, _P, _sz, ctypes.POINTER(_sz)]),
    "tdt_sigtab_import": (_i, [_P, _P, _sz]),
    "tdt_sigtab_format": (_i, [_P, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "tdt_sigtab_text": (_i, [_P, _i, _PP, ctypes.POINTER(_sz), _P]),
    "tdt_sigtab_sizes": (_i, [_P, _i, _P]),
    "tdt_sigtab_pwrite": (_i, [_P, _i, _i, _i, _i64]),
    "tdt_sigtab_cluster_table": (_i, [_P, _i, _i64, ctypes.POINTER(_sz), ctypes.POINTER(_i)]),
    "tdt_sigtab_cluster_columns": (_i, [_P, _P, _P, _P, _P, _P]),
    "tdt_sigtab_cluster_kinds": (_i, [_P, _P]),
    "tdt_sigtab_regroup": (_i, [_P, _P, ctypes.POINTER(_sz), ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "tdt_sigtab_regroup_result": (_i, [_P] * 11),
    "tdt_masked_medians": (_i, [_P, _P, _P, _P, _i, _P, _P, _P]),
    "tdt_masked_medians_parts": (_i, [_P, _P, _P, _P, _i, _P, _P, _P]),
    "tdt_window_medians": (_i, [_P, _P, _P, _i64, _P, _sz, _P, _i, _P, _P, _P]),
    "tdt_window_medians_device": (_i, [_P, _P, _P, _i64, _P, _sz, _P, _i, _P, _P, _P]),
    "tdt_gc_class_medians": (_i, [_P, _P, _P, _i64, _P, _i, _P, _P, _P]),
    "tdt_gc_class_medians_device": (_i, [_P, _P, _P, _i64, _P, _i, _P, _P, _P]),
    "tdt_cnv_bins": (_i, [_P, _P, _P, _i64, _P, _i, _P, _i, _P]),
    "tdt_cnv_bins_device": (_i, [_P, _P, _P, _i64, _P, _i, _P, _i, _P]),
    "tdt_cnv_viterbi": (_i, [_P, _P, _i64, _P, _i, _i, _i64, _i64, _P]),
    "tdt_cnv_viterbi_device": (_i, [_P, _P, _i64, _P, _i, _i, _i64, _i64, _P]),
    "tdt_ascn_emissions": (_i, [_P, _P, _P, _P, _i64, _P, _i64, _P, _i, _i, _i64, _i, _i, _i, _i, _P, _P, _P]),
    "tdt_ascn_emissions_device": (_i, [_P, _P, _P, _P, _i64, _P, _i64, _P, _i, _i, _i64, _i, _i, _i, _i, _P, _P, _P]),
    "tdt_hmm16_viterbi": (_i, [_P, _P, _i64, _P, _i, _i64, _P]),
    "tdt_hmm16_viterbi_device": (_i, [_P, _P, _i64, _P, _i, _i64, _P]),
    "tdt_segment_means": (_i, [_P, _P, _P, _i64, _P, _P, _P, _sz, _P, _P]),
    "tdt_segment_means_device": (_i, [_P, _P, _P, _P, _P, _P, _sz, _P, _P]),
    "tdt_region_counts": (_i, [_P] * 9 + [_sz, _i, _i64, _P, _P, _P, _sz, _i, _i64, _P]),
    "tdt_region_counts_device": (_i, [_P] * 9 + [_sz, _i, _i, _i64, _P, _P, _P, _sz, _i, _i64, _P]),
    "tdt_evstore_create": (_i, [_P, _i, _i, _i64, _sz, _PP]),
    "tdt_evstore_destroy": (_i, [_P]),
    "tdt_evstore_append_device": (_i, [_P] * 10 + [_sz]),
    "tdt_evstore_append": (_i, [_P] * 10 + [_sz]),
    "tdt_evstore_info": (_i, [_P, ctypes.POINTER(_sz), ctypes.POINTER(_sz), _PP]),
    "tdt_evstore_spans": (_i, [_P, _P]),
    "tdt_region_counts_packed": (_i, [_P, _P, _P, _i, _P, _sz, _i, _i64, _P]),
    "tdt_region_counts_packed_device": (_i, [_P, _P, _P, _i, _P, _sz, _i, _i64, _P]),
    "tdt_depth_dist": (_i, [_P, _P, _P, _i, _i, _P]),
    "tdt_junction_support": (_i, [_P, _P, _P, _i, _P, _sz, _i, _P]),
    "tdt_junction_support_device": (_i, [_P, _P, _P, _i, _P, _sz, _i, _P]),
    "tdt_junction_timing": (_i, [_P, ctypes.POINTER(_dbl)]),
    "tdt_links_create": (_i, [_P, _P, _P, _P, _P, _i, _PP]),
    "tdt_links_destroy": (_i, [_P]),
    "tdt_links_count": (_i, [_P, _P, _sz, _P]),
    "tdt_links_count_device": (_i, [_P, _P, _sz, _P]),
    "tdt_alleles_create": (_i, [_P, _P, _P, _i, _i, _i, _PP]),
    "tdt_alleles_destroy": (_i, [_P]),
    "tdt_alleles_reset": (_i, [_P]),
    "tdt_alleles_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_alleles_push": (_i, [_P] * 7 + [_sz, _P, _sz]),
    "tdt_alleles_counts": (_i, [_P, _P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "tdt_alleles_counts_device": (_i, [_P, _P, _P]),
    "tdt_alleles_phase_enable": (_i, [_P, _P, _sz, _sz, _i]),
    "tdt_alleles_phase_keys": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_alleles_phase_finish": (_i, [_P, _P, ctypes.c_uint64, _P]),
    "tdt_alleles_phase_sites": (_i, [_P, _P, _P, _sz]),
    "tdt_alleles_phase_blocks": (_i, [_P] * 7 + [ctypes.POINTER(_sz)]),
    "tdt_alleles_phase_links": (_i, [_P] * 6 + [ctypes.POINTER(_sz)]),
    "tdt_alleles_phase_timing": (_i, [_P, _P]),
    "tdt_alleles_phase_reserve_stats": (_i, [_P, _P]),
    "tdt_phase_forest": (_i, [_P] * 5 + [_sz, _sz, ctypes.c_uint64] + [_P] * 5),
    "tdt_phase_forest_device": (_i, [_P] * 5 + [_sz, _sz, ctypes.c_uint64] + [_P] * 5),
    "tdt_qc_create": (_i, [_P, _PP]),
    "tdt_qc_destroy": (_i, [_P]),
    "tdt_qc_reset": (_i, [_P]),
    "tdt_qc_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_qc_push": (_i, [_P] * 8 + [_sz, _P, _sz]),
    "tdt_qc_counts": (_i, [_P, _P]),
    "tdt_qc_counts_device": (_i, [_P, _P]),
    "tdt_qc_size": (_sz, []),
    "tdt_dup_create": (_i, [_P, _i, _i64, _sz, _PP]),
    "tdt_dup_destroy": (_i, [_P]),
    "tdt_dup_reset": (_i, [_P]),
    "tdt_dup_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_dup_push": (_i, [_P] * 8 + [_sz, _P, _sz]),
    "tdt_dup_keys": (_i, [_P, _P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_dup_finish": (_i, [_P, _P]),
    "tdt_dup_timing": (_i, [_P, _P]),
    "tdt_dup_size": (_sz, []),
    "tdt_indel_create": (_i, [_P, _i, _i, _sz, _PP]),
    "tdt_indel_destroy": (_i, [_P]),
    "tdt_indel_reset": (_i, [_P]),
    "tdt_indel_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_indel_push": (_i, [_P] * 6 + [_sz, _P, _sz]),
    "tdt_indel_keys": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_indel_finish": (_i, [_P, ctypes.c_uint64, _P, ctypes.POINTER(_sz)]),
    "tdt_indel_rows": (_i, [_P, _P, _P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_indel_timing": (_i, [_P, _P]),
    "tdt_indel_reserve_stats": (_i, [_P, _P]),
    "tdt_indel_sn_size": (_sz, []),
    "tdt_indel_set_reference": (_i, [_P, _P]),
    "tdt_indel_norm_stats": (_i, [_P, _P]),
    "tdt_str_create": (_i, [_P, _P, _P, _P, _P, _i, _i, _i, _sz, _PP]),
    "tdt_str_destroy": (_i, [_P]),
    "tdt_str_reset": (_i, [_P]),
    "tdt_str_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_str_push": (_i, [_P] * 7 + [_sz, _P, _sz]),
    "tdt_str_keys": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_str_finish": (_i, [_P, _P, ctypes.POINTER(_sz)]),
    "tdt_str_rows": (_i, [_P, _P, _P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_str_timing": (_i, [_P, _P]),
    "tdt_str_reserve_stats": (_i, [_P, _P]),
    "tdt_str_sn_size": (_sz, []),
    "tdt_snv_create": (_i, [_P, _i, _i, _i, _sz, _P, _PP]),
    "tdt_snv_destroy": (_i, [_P]),
    "tdt_snv_reset": (_i, [_P]),
    "tdt_snv_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_snv_push": (_i, [_P] * 6 + [_sz, _P, _sz]),
    "tdt_snv_keys": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_snv_finish": (_i, [_P, ctypes.c_uint64, _P, ctypes.POINTER(_sz)]),
    "tdt_snv_rows": (_i, [_P, _P, _P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_snv_timing": (_i, [_P, _P]),
    "tdt_snv_reserve_stats": (_i, [_P, _P]),
    "tdt_snv_sn_size": (_sz, []),
    "tdt_pile_create": (_i, [_P, _i, _P, _i, _PP]),
    "tdt_pile_destroy": (_i, [_P]),
    "tdt_pile_reset": (_i, [_P]),
    "tdt_pile_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_pile_push": (_i, [_P] * 6 + [_sz, _P, _sz]),
    "tdt_pile_finish": (_i, [_P]),
    "tdt_pile_depth": (_i, [_P, _i, _i64, _i64, _P]),
    "tdt_pile_genotype": (_i, [_P, _P, _P, _sz, _P]),
    "tdt_pile_genotype_device": (_i, [_P, _P, _P, _sz, _P]),
    "tdt_pile_counters": (_i, [_P, _P]),
    "tdt_pile_timing": (_i, [_P, _P]),
    "tdt_pile_sn_size": (_sz, []),
    "tdt_clip_create": (_i, [_P, _i, _i, _i, _sz, _PP]),
    "tdt_clip_destroy": (_i, [_P]),
    "tdt_clip_reset": (_i, [_P]),
    "tdt_clip_push_device": (_i, [_P, _P, _sz, _sz]),
    "tdt_clip_push": (_i, [_P] * 6 + [_sz, _P, _sz]),
    "tdt_clip_keys": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_clip_finish": (_i, [_P, ctypes.c_uint64, _P, ctypes.POINTER(_sz)]),
    "tdt_clip_rows": (_i, [_P] * 10 + [ctypes.POINTER(_sz)]),
    "tdt_clip_timing": (_i, [_P, _P]),
    "tdt_clip_reserve_stats": (_i, [_P, _P]),
    "tdt_clip_sn_size": (_sz, []),
    "tdt_clip_align_sites": (_i, [_P, _P, _sz] + [_P] * 4 + [_i, _i, _i] + [_P] * 5),
    "tdt_clip_align_sites_device": (_i, [_P, _P, _sz] + [_P] * 4 + [_i, _i, _i] + [_P] * 5),
    "tdt_clip_align": (_i, [_P, _P, _i, _i, _i, _P]),
    "tdt_clip_align_rows": (_i, [_P] * 6 + [ctypes.POINTER(_sz)]),
    "tdt_clip_align_timing": (_i, [_P, ctypes.POINTER(_dbl)]),
    "tdt_clip_far_sites": (_i, [_P, _P, _sz] + [_P] * 4 + [_i, _i] + [_P] * 6),
    "tdt_clip_far_sites_device": (_i, [_P, _P, _sz] + [_P] * 4 + [_i, _i] + [_P] * 6),
    "tdt_clip_far": (_i, [_P, _P, _i, _i, _P]),
    "tdt_clip_far_rows": (_i, [_P] * 7 + [ctypes.POINTER(_sz)]),
    "tdt_clip_far_timing": (_i, [_P, _P]),
    "tdt_clip_ext_enable": (_i, [_P, _sz]),
    "tdt_clip_ext_keys": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_clip_ins": (_i, [_P, _i, _i, _i, _P]),
    "tdt_clip_ext_rows": (_i, [_P, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_clip_ins_rows": (_i, [_P] * 9 + [ctypes.POINTER(_sz)]),
    "tdt_clip_ins_timing": (_i, [_P, _P]),
    "tdt_clip_ins_sites": (_i, [_P, _sz] + [_P] * 4 + [_i, _i, _i] + [_P] * 9 + [ctypes.POINTER(_sz)]),
    "tdt_clip_ins_sites_device": (_i, [_P, _sz] + [_P] * 4 + [_i, _i, _i] + [_P] * 9 + [ctypes.POINTER(_sz)]),
    "tdt_sw_align": (_i, [_P, _P, _sz, _P, _P, _i] + [_P] * 10),
    "tdt_sw_align_device": (_i, [_P, _P, _sz, _P, _P, _i] + [_P] * 10),
    "tdt_sw_align_timing": (_i, [_P]),
    "tdt_clip_mei": (_i, [_P, _P, _i, _P]),
    "tdt_clip_mei_rows": (_i, [_P] * 13 + [ctypes.POINTER(_sz)]),
    "tdt_clip_mei_timing": (_i, [_P, _P]),
    "tdt_refseq_create": (_i, [_P, _i, _P, _PP]),
    "tdt_refseq_destroy": (_i, [_P]),
    "tdt_refseq_load_fasta": (_i, [_P, _i, _P, _i64, _i64, _i, _i]),
    "tdt_refseq_load_fasta_device": (_i, [_P, _i, _P, _i64, _i64, _i, _i]),
    "tdt_refseq_fetch": (_i, [_P, _i, _i64, _i64, _P]),
    "tdt_refseq_layout": (_i, [_P, _P, _P, _P]),
    "tdt_debug_refseq_fill": (_i, [_P, _i, _i]),
    "tdt_format_coverage": (_i, [_P, _sz, ctypes.c_char_p, _i64, _i64, _i, _P, _sz, ctypes.POINTER(_sz)]),
    "tdt_fasta_write_fai": (_i, [ctypes.c_char_p, ctypes.c_char_p]),
    "tdt_host_threads": (_i, [_i]),
    "tdt_bgzf_scan": (_i, [_P, _sz, _sz, _P, _P, _P]),
    "tdt_bgzf_inflate": (_i, [_P, _sz, _P, _sz, _i]),
    "tdt_bgzf_inflate_hbm": (_i, [_P, _P, _sz, _P, _sz, _i]),
    "tdt_ingest_create": (_i, [_P, _i, _PP]),
    "tdt_ingest_destroy": (_i, [_P]),
    "tdt_ingest_push": (_i, [_P, _P, _sz, _sz, ctypes.POINTER(_sz)]),
    "tdt_ingest_push_bounded": (_i, [_P, _P, _sz, _sz, _sz, ctypes.POINTER(_sz), ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "tdt_ingest_prefetch": (_i, [_P, _P, _sz]),
    "tdt_ingest_push_ahead": (_i, [_P, _P, _sz]),
    "tdt_ingest_arrays": (_i, [_P, _PP, ctypes.POINTER(_sz)]),
    "tdt_ingest_packed": (_i, [_P, _PP]),
    "tdt_ingest_bin_for": (_i, [_P, _P, ctypes.POINTER(_i)]),
    "tdt_ingest_second_for": (_i, [_P, _P, ctypes.POINTER(_i)]),
    "tdt_ingest_packed_second": (_i, [_P, _PP]),
    "tdt_calib_stream_read": (_i, [_P, _P, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P]),
    "tdt_ingest_timing": (_i, [_P, _P]),
    "tdt_ingest_retain": (_i, [_P, _PP]),
    "tdt_ingest_edge_tids": (_i, [_P, _P, _sz]),
    "tdt_ingest_release": (_i, [_P]),
    "tdt_ingest_edges": (_i, [_P, _P, _sz, ctypes.POINTER(_sz)]),
    "tdt_ingest_carry": (_i, [_P, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "tdt_copy_to_host": (_i, [_P, _P, _P, _sz]),
    "tdt_device_cache_flush": (_i, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "tdt_device_cache_bytes": (ctypes.c_uint64, [_P]),
    "tdt_debug_fail_next_malloc": (None, [ctypes.c_int]),
    "tdt_stats_create": (_i, [_P, _i64, _i, _i64, _PP]),
    "tdt_stats_destroy": (_i, [_P]),
    "tdt_stats_push_device": (_i, [_P] * 9 + [_sz, ctypes.POINTER(_i)]),
    "tdt_stats_counts": (_i, [_P, _P]),
    "tdt_stats_moments": (_i, [_P, _dbl, _i64, _i64, ctypes.POINTER(_dbl), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "tdt_stats_scan": (_i, [_P] * 8 + [_sz, _i64, _i, _i64, _P, _P, ctypes.POINTER(_sz)]),
    "tdt_bam_decode": (_i, [_P, _sz, _sz, ctypes.POINTER(_sz), ctypes.POINTER(_sz)] + [_P] * 13),
}


def load():
    """dlopen libtiddit_hip.so and type every entry point (no GPU needed for this step)."""
    global _lib
    with _lock:
        if _lib is None:
            # PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP/HSA runtimes in
            # one process cannot both own the GPU, so when torch is installed it must be loaded first:
            # libtiddit_hip.so (NEEDED libamdhip64.so.7) then binds to the runtime torch already mapped.
            if "torch" not in sys.modules and not os.environ.get("TIDDIT_AMD_NO_TORCH"):
                try:
                    import torch  # noqa: F401
                except ImportError:
                    pass
            if not os.path.exists(SO_PATH):
                raise ImportError("libtiddit_hip.so is not built (run `python -m tiddit_amd.build`); "
                                  "tiddit_amd has no CPU fallback")
            L = ctypes.CDLL(SO_PATH)
            for name, (res, args) in SYMBOLS.items():
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
            # a measurement build (ablation / tunable macros, tools/build_variant.sh) is never what the product runs by accident
            flags = L.tdt_build_flags().decode()
            if flags and os.environ.get("TIDDIT_ALLOW_VARIANT") != "1":
                raise ImportError("%s was built with measurement macros (%s); set TIDDIT_ALLOW_VARIANT=1 to load it anyway" % (SO_PATH, flags))
            _lib = L
    return _lib


def check(rc):
    if rc != TDT_OK:
        raise TdtError(rc, load().tdt_last_error().decode(errors="replace"))


def ptr(a):
    """host numpy array -> void*"""
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Context:
    """One tdt_ctx (device + stream + scratch).  Contexts are per process; use default_context()."""

    def __init__(self, device=0):
        self.lib = load()
        h = ctypes.c_void_p()
        check(self.lib.tdt_ctx_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device

    def sync(self):
        check(self.lib.tdt_ctx_sync(self.handle))

    def set_stream(self, hip_stream):
        check(self.lib.tdt_ctx_set_stream(self.handle, ctypes.c_void_p(hip_stream)))

    def close(self):
        if self.handle:
            self.lib.tdt_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = {}


def default_context(device=None):
    if device is None:
        device = int(os.environ.get("TIDDIT_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    key = (os.getpid(), device)
    if key not in _default:
        _default[key] = Context(device)
    return _default[key]
