"""hpg-variant_amd -- MI355X-native per-variant statistics engine for HPG Variant.

Python is plumbing here: this module only loads the C-ABI shared library
(include/hpgv.h) with ctypes and gives numpy-friendly wrappers for the tests
and bench.  There is no CPU implementation behind it: if the HIP library is
missing or no device is present, calls raise.

The directory name has a hyphen, so import it with
    importlib.import_module("hpg-variant_amd")
"""
import ctypes as C
import os

import numpy as np

from . import _build

OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_STATE, ERR_UNSUPPORTED = 1, 2, 3, 4, 5, 6
TASK_CHISQ, TASK_FISHER = 1, 2
EPI_TESTING, EPI_TRAINING = 0, 1
# the scan kernel a ranking call ran (hpgv_epi_last_rank_info; HPGV_EPI_KERNEL_* of include/hpgv.h)
(EPI_KERNEL_NONE, EPI_KERNEL_PAIRS_MFMA, EPI_KERNEL_PAIRS_VALU, EPI_KERNEL_TRIPLES_MFMA, EPI_KERNEL_TRIPLES3, EPI_KERNEL_TRIPLES1,
 EPI_KERNEL_TRIPLES, EPI_KERNEL_COMBS, EPI_KERNEL_COMBS_WIDE) = range(9)
EPI_KERNEL_NAMES = {EPI_KERNEL_NONE: "none", EPI_KERNEL_PAIRS_MFMA: "k_epi_pairs_mfma", EPI_KERNEL_PAIRS_VALU: "k_epi_pairs",
                    EPI_KERNEL_TRIPLES_MFMA: "k_epi_triples_mfma", EPI_KERNEL_TRIPLES3: "k_epi_triples3",
                    EPI_KERNEL_TRIPLES1: "k_epi_triples1", EPI_KERNEL_TRIPLES: "k_epi_triples", EPI_KERNEL_COMBS: "k_epi_combs",
                    EPI_KERNEL_COMBS_WIDE: "k_epi_combs_wide"}
COND_UNAFFECTED, COND_AFFECTED, COND_OTHER = 0, 1, 2
SEX_MALE, SEX_FEMALE, SEX_UNKNOWN = 0, 1, 2
# the model tests' order in chisq5 / p5 (HPGV_MODEL_* of include/hpgv.h)
MODEL_GENO, MODEL_TREND, MODEL_ALLELIC, MODEL_DOM, MODEL_REC = range(5)
# the logistic regression's limits and row status (HPGV_LOGISTIC_MAX_COVAR, HPGV_LOGIT_* of include/hpgv.h)
LOGISTIC_MAX_COVAR = 14
LOGIT_OK, LOGIT_NOT_CONVERGED, LOGIT_SINGULAR = 0, 1, 2
# the linear regression's row status (HPGV_LINEAR_* of include/hpgv.h)
LINEAR_OK, LINEAR_SINGULAR, LINEAR_EXACT = 0, 1, 2
LAYOUT_ASSOC, LAYOUT_TDT, LAYOUT_STATS, LAYOUT_STATS_GROUPS, LAYOUT_MENDEL, LAYOUT_EPI = 0, 1, 2, 3, 4, 5
GT_MISSING = 0xFF
# the tokenizer's tile records that hpgv_bgzf_verify_tiles_dev leaves (csrc/hpgv_text2_kernels.h: TOK2_TILE, struct TokAgg2 { TokAgg
# h[2]; }, struct TokAgg { int nl, tabs, last_nl, pad; }, enum TOK_AGG_*): one 32-byte record per 2 KiB tile of the decoded text, two
# 16-byte halves of four 32-bit words each, the flags in the last word (pad) of a half; "count this tile again" is OR-ed into h[0]'s.
# test_tile_record_constants_match_the_kernels_header holds them to the header.
TOK_TILE_BYTES = 2048
TOK_TILE_RECORD_BYTES, TOK_TILE_HALF_WORDS = 32, 4
TOK_AGG_NL, TOK_AGG_TABS, TOK_AGG_LAST_NL, TOK_AGG_PAD = 0, 1, 2, 3
TOK_AGG_WRITTEN, TOK_AGG_COMPLEX = 1, 2

# every symbol include/hpgv.h declares (checked by the CPU suite)
SYMBOLS = [
    "hpgv_version", "hpgv_device_count", "hpgv_create", "hpgv_create_multi", "hpgv_group_size", "hpgv_group_member", "hpgv_member_device", "hpgv_destroy", "hpgv_last_error",
    "hpgv_set_option", "hpgv_set_cohort", "hpgv_assoc_layout", "hpgv_set_families",
    "hpgv_tdt_layout", "hpgv_set_logfact", "hpgv_set_stats_cohort", "hpgv_stats_layout",
    "hpgv_set_stats_groups", "hpgv_stats_groups_layout", "hpgv_stats_scan_group_dev",
    "hpgv_set_pedigree", "hpgv_mendel_layout", "hpgv_mendel_scan_dev", "hpgv_mendel_children_dev",
    "hpgv_dev_alloc", "hpgv_dev_free", "hpgv_memcpy_h2d", "hpgv_memcpy_d2h", "hpgv_stream_sync",
    "hpgv_device_numa_node", "hpgv_memcpy_h2d_async", "hpgv_inflate_blocks_dev", "hpgv_bgzf_verify_dev", "hpgv_bgzf_scan_dev", "hpgv_bgzf_scan_scratch_bytes", "hpgv_dev_reserve", "hpgv_dev_commit", "hpgv_dev_committed", "hpgv_dev_release", "hpgv_text_alias", "hpgv_stream_create", "hpgv_stream_create_low", "hpgv_stream_destroy", "hpgv_host_alloc", "hpgv_host_free",
    "hpgv_layout_dev", "hpgv_synth_dev", "hpgv_synth_raw_dev",
    "hpgv_assoc_scan_dev", "hpgv_assoc_chisq_dev", "hpgv_assoc_fisher_dev",
    "hpgv_tdt_scan_dev", "hpgv_tdt_stats_dev", "hpgv_stats_scan_dev", "hpgv_stats_hwe_dev",
    "hpgv_sample_missing_dev", "hpgv_genotype_table_dev", "hpgv_stats_filter_dev",
    "hpgv_mendel", "hpgv_epi_dataset", "hpgv_tokenize_dev", "hpgv_tokenize", "hpgv_assoc_text", "hpgv_tdt_text",
    "hpgv_last_kernel_ms", "hpgv_assoc", "hpgv_tdt", "hpgv_stats", "hpgv_stats_ex", "hpgv_stats_groups",
    "hpgv_epi_dataset_text", "hpgv_set_text_filters", "hpgv_stats_text", "hpgv_stats_text_groups", "hpgv_epi_set_dataset", "hpgv_epi_set_folds", "hpgv_epi_set_fold_masks", "hpgv_epi_counts",
    "hpgv_epi_counts_all_folds", "hpgv_epi_scan_pairs", "hpgv_epi_rank_pairs", "hpgv_epi_rank_pairs_rows", "hpgv_epi_scan_triples", "hpgv_epi_rank_triples", "hpgv_epi_eval_combs", "hpgv_epi_rank_order", "hpgv_epi_rank_order_rows", "hpgv_read_probe",
    "hpgv_group_comm_init", "hpgv_group_comm_ranks", "hpgv_group_rccl_probe", "hpgv_group_shard", "hpgv_group_assoc", "hpgv_group_tdt", "hpgv_group_stats", "hpgv_group_sync", "hpgv_group_epi_share", "hpgv_group_epi_rank", "hpgv_epi_rank_triples_rows", "hpgv_text_alias_tiles", "hpgv_text_tiles_bytes", "hpgv_bgzf_verify_tiles_dev", "hpgv_memset_dev",
    "hpgv_epi_last_rank_info", "hpgv_filter_text", "hpgv_text_partition", "hpgv_lines_partition_scratch_bytes", "hpgv_lines_partition_dev",
    "hpgv_text_multisplit", "hpgv_lines_multisplit_scratch_bytes", "hpgv_lines_multisplit_dev",
    "hpgv_inheritance_scan_dev", "hpgv_set_text_inheritance_filters",
    "hpgv_bgzf_deflate_bound", "hpgv_bgzf_deflate_scratch_bytes", "hpgv_bgzf_deflate_dev", "hpgv_bgzf_compress",
    "hpgv_text_partition_bgzf", "hpgv_text_multisplit_bgzf",
    "hpgv_set_perm_labels", "hpgv_assoc_perm_dev", "hpgv_assoc_perm", "hpgv_assoc_perm_text", "hpgv_perm_labels_shuffle", "hpgv_perm_pvalues",
    "hpgv_set_tdt_flips", "hpgv_tdt_perm_dev", "hpgv_tdt_perm", "hpgv_tdt_perm_text", "hpgv_perm_flips_shuffle",
    "hpgv_assoc_model_scan_dev", "hpgv_assoc_model_stats_dev", "hpgv_assoc_trend_perm_dev", "hpgv_assoc_model", "hpgv_assoc_model_text",
    "hpgv_set_strata", "hpgv_assoc_cmh_dev", "hpgv_assoc_cmh", "hpgv_assoc_cmh_text", "hpgv_cmh_fit",
    "hpgv_assoc_cmh_perm_dev", "hpgv_assoc_cmh_perm", "hpgv_assoc_cmh_perm_text", "hpgv_perm_labels_shuffle_within",
    "hpgv_set_covariates", "hpgv_assoc_logistic_dev", "hpgv_assoc_logistic", "hpgv_assoc_logistic_text", "hpgv_logistic_fit",
    "hpgv_set_phenotype", "hpgv_assoc_linear_dev", "hpgv_assoc_linear", "hpgv_assoc_linear_text", "hpgv_linear_fit", "hpgv_linear_t_p",
    "hpgv_perm_order_shuffle", "hpgv_set_linear_perms", "hpgv_assoc_linear_perm_dev", "hpgv_assoc_linear_perm", "hpgv_assoc_linear_perm_text", "hpgv_linear_perm_fit", "hpgv_mfma_f64_probe",
    "hpgv_ld_window_dev", "hpgv_ld", "hpgv_ld_text", "hpgv_ld_r2",
    "hpgv_ld_edges_dev", "hpgv_ld_edges", "hpgv_clump",
    "hpgv_rows_gather_scratch_bytes", "hpgv_rows_gather_dev", "hpgv_assoc_select_text",
    "hpgv_ibs_pairs_dev", "hpgv_ibs_class_counts_dev", "hpgv_ibs_select_dev", "hpgv_ibs", "hpgv_ibs_text", "hpgv_ibs_terms", "hpgv_ibs_genome",
    "hpgv_ibs_plan_rows",
    "hpgv_grm_table_dev", "hpgv_grm_pairs_dev", "hpgv_grm", "hpgv_grm_text", "hpgv_grm_table", "hpgv_grm_frac_bits", "hpgv_grm_value", "hpgv_grm_plan_rows",
    "hpgv_grm_matrix_dev", "hpgv_pca_apply_dev", "hpgv_pca_dev", "hpgv_pca_block", "hpgv_pca_jacobi", "hpgv_pca_chol_inv",
    "hpgv_score_table_dev", "hpgv_score_cols_dev", "hpgv_score", "hpgv_score_text", "hpgv_score_table", "hpgv_score_frac_bits", "hpgv_score_value",
    "hpgv_score_plan_rows",
]

# hpgv_ld_edge: {int32 a, b; double r2}, 16 bytes
LD_EDGE = np.dtype([("a", np.int32), ("b", np.int32), ("r2", np.float64)])
# hpgv_ibs_counts: {int32 n, ibs0, ibs1, ibs2}, 16 bytes; hpgv_ibs_pair: {int32 i, j; hpgv_ibs_counts c; double pi_hat}, 32 bytes
IBS_COUNTS = np.dtype([("n", np.int32), ("ibs0", np.int32), ("ibs1", np.int32), ("ibs2", np.int32)])
IBS_PAIR = np.dtype([("i", np.int32), ("j", np.int32), ("c", IBS_COUNTS), ("pi_hat", np.float64)])
# hpgv_grm_acc: {int64 sq, n}, 16 bytes; a row's table record of hpgv_grm_table_dev: {int8 hi[4], lo[4]}, 8 bytes
GRM_ACC = np.dtype([("sq", np.int64), ("n", np.int64)])
GRM_TAB = np.dtype([("hi", np.int8, 4), ("lo", np.int8, 4)])
# "Score" of include/hpgv.h: the most scores per call, a row's flag bits, and hpgv_score_text's callback
SCORE_MAX = 32
SCORE_SKIP, SCORE_FLIP = 1, 2
SCORE_WEIGH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                             C.POINTER(C.c_double), C.POINTER(C.c_uint8))
# hpgv_logistic_result: {double beta, se, stat, p; int32 n_obs, iters, status, pad}, 48 bytes
LOGISTIC_RESULT = np.dtype([("beta", np.float64), ("se", np.float64), ("stat", np.float64), ("p", np.float64),
                            ("n_obs", np.int32), ("iters", np.int32), ("status", np.int32), ("pad", np.int32)])
# hpgv_cmh_result: {int32 n_strata_cmh, n_strata_bd; double chisq, p, or_mh, se, l95, u95, chisq_bd, p_bd}, 72 bytes
CMH_RESULT = np.dtype([("n_strata_cmh", np.int32), ("n_strata_bd", np.int32), ("chisq", np.float64), ("p", np.float64), ("or_mh", np.float64),
                       ("se", np.float64), ("l95", np.float64), ("u95", np.float64), ("chisq_bd", np.float64), ("p_bd", np.float64)])
CMH_MAX_STRATA = 1024               # HPGV_CMH_MAX_STRATA
# hpgv_linear_result: {double beta, se, stat, p; int32 n_obs, df, status, pad}, 48 bytes
LINEAR_RESULT = np.dtype([("beta", np.float64), ("se", np.float64), ("stat", np.float64), ("p", np.float64),
                          ("n_obs", np.int32), ("df", np.int32), ("status", np.int32), ("pad", np.int32)])


class HpgvError(RuntimeError):
    pass


class EpiRankInfo(C.Structure):
    """hpgv_epi_rank_info"""
    _fields_ = [("kernel", C.c_int32), ("launches", C.c_int32), ("relaunches", C.c_int32), ("reserved", C.c_int32)]


_lib = None


def build(force=False, verbose=False):
    _build.build_all(force=force, verbose=verbose)


def lib_path():
    """libhpgv.so of this tree; HPGV_LIB names another build of it (tools/build_ablation.py: the forms that lost their A/B)."""
    return os.environ.get("HPGV_LIB") or _build.LIB


def load():
    """Loads libhpgv.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise HpgvError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                        "there is no CPU fallback" % path)
    L = C.CDLL(path)
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    L.hpgv_version.restype = C.c_char_p
    L.hpgv_last_error.restype = C.c_char_p
    L.hpgv_last_error.argtypes = [vp]
    L.hpgv_create.argtypes = [i32, C.POINTER(vp)]
    L.hpgv_create_multi.argtypes = [vp, i32, C.POINTER(vp)]
    L.hpgv_group_size.argtypes = [vp]
    L.hpgv_group_member.argtypes = [vp, i32]
    L.hpgv_group_member.restype = vp
    L.hpgv_member_device.argtypes = [vp, i32]
    L.hpgv_destroy.argtypes = [vp]
    L.hpgv_destroy.restype = None
    L.hpgv_set_option.argtypes = [vp, C.c_char_p, C.c_long]
    L.hpgv_set_cohort.argtypes = [vp, vp, i32]
    L.hpgv_assoc_layout.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]
    L.hpgv_set_families.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.hpgv_tdt_layout.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]
    L.hpgv_set_logfact.argtypes = [vp, vp, sz]
    L.hpgv_set_stats_cohort.argtypes = [vp, i32]
    L.hpgv_stats_layout.argtypes = [vp, C.POINTER(sz)]
    L.hpgv_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.hpgv_dev_free.argtypes = [vp, vp]
    L.hpgv_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.hpgv_host_free.argtypes = [vp, vp]
    L.hpgv_memcpy_h2d.argtypes = [vp, vp, vp, sz, vp]
    L.hpgv_memcpy_d2h.argtypes = [vp, vp, vp, sz, vp]
    L.hpgv_stream_sync.argtypes = [vp, vp]
    L.hpgv_layout_dev.argtypes = [vp, i32, vp, sz, i32, vp, vp]
    L.hpgv_synth_dev.argtypes = [vp, i32, u64, i32, vp, vp]
    L.hpgv_synth_raw_dev.argtypes = [vp, u64, i32, i32, sz, vp, vp]
    L.hpgv_assoc_scan_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_assoc_chisq_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.hpgv_assoc_fisher_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_tdt_scan_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_tdt_stats_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.hpgv_stats_scan_dev.argtypes = [vp, vp, i32, vp, vp]
    L.hpgv_stats_hwe_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.hpgv_assoc.argtypes = [vp, i32, vp, sz, i32, vp] + [vp] * 7
    L.hpgv_tdt.argtypes = [vp, vp, sz, i32, vp] + [vp] * 5
    L.hpgv_stats.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    L.hpgv_stats_ex.argtypes = [vp, vp, sz, i32, vp, vp, vp, vp, vp, vp, C.POINTER(i32)]
    L.hpgv_stats_groups.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    L.hpgv_sample_missing_dev.argtypes = [vp, vp, i32, vp, vp]
    L.hpgv_genotype_table_dev.argtypes = [vp, vp, sz, i32, vp, i32, vp, vp]
    L.hpgv_tokenize_dev.argtypes = [vp, vp, sz, i32, i32, i32, vp, vp, vp, vp, sz, vp, vp, vp]
    L.hpgv_inflate_blocks_dev.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.hpgv_bgzf_verify_dev.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.hpgv_bgzf_verify_tiles_dev.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, u64, vp]
    L.hpgv_text_tiles_bytes.restype = sz
    L.hpgv_text_tiles_bytes.argtypes = [u64]
    L.hpgv_text_alias_tiles.argtypes = [vp, vp, vp, vp, vp, u64]
    L.hpgv_bgzf_scan_scratch_bytes.argtypes = [u64, i32]
    L.hpgv_bgzf_scan_scratch_bytes.restype = sz
    L.hpgv_bgzf_scan_dev.argtypes = [vp, vp, u64, u64, u64, i32, vp, vp, vp, vp, vp, sz, vp, vp]
    L.hpgv_dev_reserve.argtypes = [vp, sz, C.POINTER(vp)]
    L.hpgv_dev_commit.argtypes = [vp, vp, sz]
    L.hpgv_dev_release.argtypes = [vp, vp]
    L.hpgv_dev_committed.argtypes = [vp, vp, C.POINTER(sz)]
    L.hpgv_tokenize.argtypes = [vp, C.c_char_p, sz, i32, i32, i32, C.POINTER(i32), vp, vp, vp, sz, vp, vp]
    L.hpgv_assoc_text.argtypes = [vp, i32, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp] + [vp] * 7
    L.hpgv_tdt_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp] + [vp] * 5
    L.hpgv_stats_filter_dev.argtypes = [vp, vp, i32, C.c_double, C.c_double, C.c_double, vp, vp]
    L.hpgv_set_stats_groups.argtypes = [vp, vp, i32, i32]
    L.hpgv_stats_groups_layout.argtypes = [vp, C.POINTER(sz), vp]
    L.hpgv_stats_scan_group_dev.argtypes = [vp, vp, i32, i32, vp, vp]
    L.hpgv_set_pedigree.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.hpgv_mendel_layout.argtypes = [vp, C.POINTER(sz)]
    L.hpgv_mendel_scan_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_mendel_children_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_mendel.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    L.hpgv_epi_dataset.argtypes = [vp, vp, sz, i32, vp]
    L.hpgv_stats_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), vp, vp]
    L.hpgv_stats_text_groups.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), vp, vp, vp, vp, vp]
    L.hpgv_set_text_filters.argtypes = [vp, C.c_double, C.c_double, C.c_long]
    L.hpgv_set_text_inheritance_filters.argtypes = [vp, C.c_double, C.c_double]
    L.hpgv_inheritance_scan_dev.argtypes = [vp, vp, i32, vp, vp]
    L.hpgv_epi_dataset_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp]
    L.hpgv_epi_set_dataset.argtypes = [vp, vp, i32, i32, i32]
    L.hpgv_epi_set_folds.argtypes = [vp, vp, i32]
    L.hpgv_epi_set_fold_masks.argtypes = [vp, vp, i32]
    L.hpgv_epi_counts.argtypes = [vp, i32, vp, i32, vp, vp]
    L.hpgv_epi_counts_all_folds.argtypes = [vp, i32, vp, i32, vp, vp]
    L.hpgv_epi_scan_pairs.argtypes = [vp, i32, i32, i32, vp, vp, C.POINTER(C.c_ulonglong)]
    L.hpgv_epi_rank_pairs.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_epi_scan_triples.argtypes = [vp, i32, vp, vp]
    L.hpgv_epi_rank_triples.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_epi_eval_combs.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    L.hpgv_epi_rank_order.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_epi_rank_order_rows.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_epi_rank_pairs_rows.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_read_probe.argtypes = [vp, vp, sz, i32, C.POINTER(C.c_float)]
    i64 = C.c_int64
    L.hpgv_group_comm_init.argtypes = [vp]
    L.hpgv_group_comm_ranks.argtypes = [vp]
    L.hpgv_group_rccl_probe.argtypes = [C.c_char_p, C.c_size_t]
    L.hpgv_group_shard.argtypes = [vp, i64, i32, C.POINTER(i64), C.POINTER(i64)]
    L.hpgv_group_assoc.argtypes = [vp, i32, vp, vp, i64, vp, vp, vp, vp]
    L.hpgv_group_tdt.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp]
    L.hpgv_group_stats.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.hpgv_group_sync.argtypes = [vp]
    L.hpgv_group_epi_share.argtypes = [vp, i32, i32, vp, vp]
    L.hpgv_group_epi_rank.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_epi_rank_triples_rows.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.hpgv_epi_last_rank_info.argtypes = [vp, C.POINTER(EpiRankInfo)]
    L.hpgv_bgzf_deflate_bound.argtypes = [u64, i32]
    L.hpgv_bgzf_deflate_bound.restype = sz
    L.hpgv_bgzf_deflate_scratch_bytes.argtypes = [u64, i32]
    L.hpgv_bgzf_deflate_scratch_bytes.restype = sz
    L.hpgv_bgzf_deflate_dev.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    L.hpgv_bgzf_compress.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.hpgv_text_partition_bgzf.argtypes = [vp, vp, vp, i32, vp, sz, i32, vp, vp, vp, vp]
    L.hpgv_text_multisplit_bgzf.argtypes = [vp, vp, vp, i32, i32, i32, vp, sz, vp, vp]
    L.hpgv_set_perm_labels.argtypes = [vp, vp, i32]
    L.hpgv_assoc_perm_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hpgv_assoc_perm.argtypes = [vp, vp, sz, i32, vp] + [vp] * 9
    L.hpgv_assoc_perm_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp] + [vp] * 9
    L.hpgv_perm_labels_shuffle.argtypes = [vp, i32, i32, u64, vp]
    L.hpgv_perm_pvalues.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    L.hpgv_set_tdt_flips.argtypes = [vp, vp, i32]
    L.hpgv_tdt_perm_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hpgv_tdt_perm.argtypes = [vp, vp, sz, i32, vp] + [vp] * 7
    L.hpgv_tdt_perm_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp] + [vp] * 7
    L.hpgv_perm_flips_shuffle.argtypes = [i32, i32, u64, vp]
    L.hpgv_assoc_model_scan_dev.argtypes = [vp, vp, i32, vp, vp]
    L.hpgv_assoc_model_stats_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_assoc_trend_perm_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.hpgv_assoc_model.argtypes = [vp, vp, sz, i32] + [vp] * 5
    L.hpgv_assoc_model_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp] + [vp] * 5
    L.hpgv_set_covariates.argtypes = [vp, vp, i32, i32]
    L.hpgv_set_strata.argtypes = [vp, vp, i32, i32]
    L.hpgv_assoc_cmh_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.hpgv_assoc_cmh.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    L.hpgv_assoc_cmh_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp]
    L.hpgv_cmh_fit.argtypes = [vp, i32, vp]
    L.hpgv_assoc_cmh_perm_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hpgv_assoc_cmh_perm.argtypes = [vp, vp, sz, i32, vp, vp, vp, vp]
    L.hpgv_assoc_cmh_perm_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp, vp]
    L.hpgv_perm_labels_shuffle_within.argtypes = [vp, vp, i32, i32, u64, vp]
    L.hpgv_assoc_logistic_dev.argtypes = [vp, vp, i32, i32, C.c_double, vp, vp, vp]
    L.hpgv_assoc_logistic.argtypes = [vp, vp, sz, i32, i32, C.c_double, vp, vp]
    L.hpgv_assoc_logistic_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, i32, C.c_double, vp, vp]
    L.hpgv_logistic_fit.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, vp, vp]
    L.hpgv_set_phenotype.argtypes = [vp, vp, i32]
    L.hpgv_assoc_linear_dev.argtypes = [vp, vp, i32, vp, vp, vp]
    L.hpgv_assoc_linear.argtypes = [vp, vp, sz, i32, vp, vp]
    L.hpgv_assoc_linear_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp]
    L.hpgv_linear_fit.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    L.hpgv_linear_t_p.argtypes = [C.c_double, i32]
    L.hpgv_linear_t_p.restype = C.c_double
    L.hpgv_perm_order_shuffle.argtypes = [vp, i32, i32, u64, vp]
    L.hpgv_set_linear_perms.argtypes = [vp, vp, i32]
    L.hpgv_assoc_linear_perm_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.hpgv_assoc_linear_perm.argtypes = [vp, vp, sz, i32, vp, vp, vp, vp]
    L.hpgv_assoc_linear_perm_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp, vp, vp]
    L.hpgv_linear_perm_fit.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp]
    L.hpgv_mfma_f64_probe.argtypes = [vp, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.hpgv_ld_window_dev.argtypes = [vp, vp, sz, i32, i32, i32, vp, vp, C.c_int64, vp, vp, vp, vp]
    L.hpgv_ld.argtypes = [vp, vp, sz, i32, i32, vp, vp, C.c_int64, vp, vp]
    L.hpgv_ld_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, i32, vp, vp]
    L.hpgv_ld_r2.argtypes = [vp]
    L.hpgv_ld_r2.restype = C.c_double
    L.hpgv_ld_edges_dev.argtypes = [vp, vp, sz, i32, i32, i32, vp, vp, C.c_int64, vp, C.c_double, vp, u64, vp, vp]
    L.hpgv_ld_edges.argtypes = [vp, vp, sz, i32, i32, vp, vp, C.c_int64, C.c_double, vp, u64, vp]
    L.hpgv_clump.argtypes = [i32, vp, vp, u64, C.c_double, vp, vp, C.POINTER(i32)]
    L.hpgv_memset_dev.argtypes = [vp, vp, i32, sz, vp]
    L.hpgv_ibs_pairs_dev.argtypes = [vp, vp, sz, i32, i32, vp, vp, vp]
    L.hpgv_ibs_class_counts_dev.argtypes = [vp, vp, sz, i32, i32, vp, vp, vp]
    L.hpgv_ibs_select_dev.argtypes = [vp, vp, i32, vp, C.c_double, vp, u64, vp, vp]
    L.hpgv_ibs.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    L.hpgv_ibs_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, vp, vp]
    L.hpgv_ibs_terms.argtypes = [i32, i32, i32, vp]
    L.hpgv_ibs_genome.argtypes = [vp, vp, vp]
    L.hpgv_ibs_genome.restype = None
    L.hpgv_ibs_plan_rows.argtypes = [i32, i32, i32]
    L.hpgv_grm_table_dev.argtypes = [vp, vp, i32, i32, C.c_double, vp, vp, vp, vp]
    L.hpgv_grm_pairs_dev.argtypes = [vp, vp, sz, i32, i32, vp, vp, vp, vp]
    L.hpgv_grm.argtypes = [vp, vp, sz, i32, vp, i32, C.c_double, vp, vp]
    L.hpgv_grm_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, i32, C.c_double, vp, vp]
    L.hpgv_grm_table.argtypes = [i32, i32, i32, i32, C.c_double, vp, vp]
    L.hpgv_grm_frac_bits.argtypes = [C.c_double]
    L.hpgv_grm_value.argtypes = [vp, i32]
    L.hpgv_grm_value.restype = C.c_double
    L.hpgv_grm_plan_rows.argtypes = [i32, i32, i32]
    L.hpgv_grm_matrix_dev.argtypes = [vp, vp, i32, i32, vp, sz, vp, vp]
    L.hpgv_score_table_dev.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, sz, vp, vp]
    L.hpgv_score_cols_dev.argtypes = [vp, vp, sz, i32, i32, vp, vp, sz, i32, vp, sz, vp]
    L.hpgv_score.argtypes = [vp, vp, sz, i32, vp, vp, i32, vp, i32, vp, vp, sz, vp]
    L.hpgv_score_text.argtypes = [vp, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp, SCORE_WEIGH_FN, vp, i32, vp, i32, vp, vp, sz, vp]
    L.hpgv_score_table.argtypes = [i32, i32, i32, vp, i32, vp, i32, i32, vp, vp]
    L.hpgv_score_frac_bits.argtypes = [C.c_double]
    L.hpgv_score_value.argtypes = [C.c_int64, C.c_int64, i32]
    L.hpgv_score_value.restype = C.c_double
    L.hpgv_score_plan_rows.argtypes = [i32, i32, i32, i32]
    L.hpgv_pca_apply_dev.argtypes = [vp, vp, i32, sz, vp, i32, vp, vp]
    L.hpgv_pca_dev.argtypes = [vp, vp, i32, sz, i32, C.c_double, i32, u64, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.hpgv_pca_block.argtypes = [i32]
    L.hpgv_pca_jacobi.argtypes = [i32, vp, vp]
    L.hpgv_pca_chol_inv.argtypes = [i32, vp, vp]
    L.hpgv_rows_gather_scratch_bytes.argtypes = [i32]
    L.hpgv_rows_gather_scratch_bytes.restype = sz
    L.hpgv_rows_gather_dev.argtypes = [vp, vp, sz, sz, i32, vp, vp, sz, vp, vp, vp, vp]
    L.hpgv_assoc_select_text.argtypes = [vp, i32, C.c_char_p, sz, i32, C.POINTER(i32), vp, vp, vp] + [vp] * 7 + \
                                        [C.c_double, vp, vp, sz, i32, C.POINTER(i32)]
    _lib = L
    return L


def perm_labels_shuffle(condition, n_perms, seed):
    """hpgv_perm_labels_shuffle: (n_perms, n_samples) uint8 label rows, each a uniform shuffle of the cohort columns'
    conditions; deterministic in (seed, row).  No device needed."""
    c = _np(condition, np.uint8)
    out = np.zeros((n_perms, len(c)), np.uint8)
    rc = load().hpgv_perm_labels_shuffle(_ptr(c), len(c), n_perms, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out))
    if rc != OK:
        raise HpgvError("hpgv_perm_labels_shuffle -> %d" % rc)
    return out


def perm_labels_shuffle_within(condition, stratum, n_perms, seed):
    """hpgv_perm_labels_shuffle_within: (n_perms, n_samples) uint8 label rows, the cohort columns' conditions shuffled inside
    every stratum (stratum (n_samples,) int32, negative = in no stratum: the observed label stays); deterministic in (seed, row).
    No device needed."""
    c, st = _np(condition, np.uint8), _np(stratum, np.int32)
    assert len(c) == len(st)
    out = np.zeros((n_perms, len(c)), np.uint8)
    rc = load().hpgv_perm_labels_shuffle_within(_ptr(c), _ptr(st), len(c), n_perms, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out))
    if rc != OK:
        e = HpgvError("hpgv_perm_labels_shuffle_within -> %d" % rc)
        e.code = rc
        raise e
    return out


def perm_order_shuffle(condition, n_perms, seed):
    """hpgv_perm_order_shuffle: (n_perms, n_samples) int32 rows, row p column j = the VCF column whose residual column j takes: a
    uniform shuffle of the cohort columns among themselves, OTHER columns fixed; deterministic in (seed, row).  No device needed."""
    c = _np(condition, np.uint8)
    out = np.zeros((n_perms, len(c)), np.int32)
    rc = load().hpgv_perm_order_shuffle(_ptr(c), len(c), n_perms, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out))
    if rc != OK:
        raise HpgvError("hpgv_perm_order_shuffle -> %d" % rc)
    return out


def perm_flips_shuffle(n_families, n_perms, seed):
    """hpgv_perm_flips_shuffle: (n_perms, n_families) uint8 flip rows, every family flipped with probability 1/2;
    deterministic in (seed, row, family).  No device needed."""
    out = np.zeros((n_perms, n_families), np.uint8)
    rc = load().hpgv_perm_flips_shuffle(n_families, n_perms, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out))
    if rc != OK:
        raise HpgvError("hpgv_perm_flips_shuffle -> %d" % rc)
    return out


def run_tdt_perm(vcf_path, ped_path, out_path, n_perms, seed, batch_bytes=1 << 22):
    """hpgv_run_tdt_perm of libhpgv_host.so (include/hpgv_host.h): the .tdt file of hpgv_run_tdt at out_path and EMP1 / EMP2 by
    family flips in out_path + ".mperm".  Returns the number of variants written."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_tdt_perm.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_size_t, C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n = C.c_long(0)
    rc = H.hpgv_run_tdt_perm(os.fsencode(vcf_path), os.fsencode(ped_path), os.fsencode(out_path), n_perms,
                             int(seed) & 0xFFFFFFFFFFFFFFFF, batch_bytes, C.byref(n))
    if rc != OK:
        raise HpgvError("hpgv_run_tdt_perm -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
    return n.value


def run_assoc_model(vcf_path, ped_path, out_path, n_perms=0, seed=0, batch_bytes=1 << 22):
    """hpgv_run_assoc_model of libhpgv_host.so (include/hpgv_host.h): the model tests' file at out_path and, with n_perms >= 1,
    EMP1 / EMP2 of the trend statistic in out_path + ".mperm".  Paths may be None (the call then fails with ERR_INVALID).
    Returns the number of variants written."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_model.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_size_t, C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n = C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_model(enc(vcf_path), enc(ped_path), enc(out_path), n_perms, int(seed) & 0xFFFFFFFFFFFFFFFF, batch_bytes, C.byref(n))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_model -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value


def run_assoc_logistic(vcf_path, ped_path, covar_path, out_path, n_covar=0, batch_bytes=1 << 22):
    """hpgv_run_assoc_logistic of libhpgv_host.so (include/hpgv_host.h): one logistic regression per variant with the first n_covar
    value columns of the covariate file (0: all of them; covar_path None: no covariates) at out_path.  Paths may be None (the call
    then fails with ERR_INVALID).  Returns (variants written, cohort samples used)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_logistic.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, used = C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_logistic(enc(vcf_path), enc(ped_path), enc(covar_path), n_covar, enc(out_path), batch_bytes, C.byref(n), C.byref(used))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_logistic -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, used.value


def run_assoc_cmh(vcf_path, ped_path, within_path, out_path, batch_bytes=1 << 22):
    """hpgv_run_assoc_cmh of libhpgv_host.so (include/hpgv_host.h): the stratified association test per variant over the strata of
    the within file at out_path.  Paths may be None (the call then fails with ERR_INVALID).  Returns (variants written, cohort
    samples used, strata)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_cmh.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, used, k = C.c_long(0), C.c_long(0), C.c_int(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_cmh(enc(vcf_path), enc(ped_path), enc(within_path), enc(out_path), batch_bytes, C.byref(n), C.byref(used), C.byref(k))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_cmh -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, used.value, k.value


def run_assoc_cmh_perm(vcf_path, ped_path, within_path, out_path, n_perms, seed, batch_bytes=1 << 22):
    """hpgv_run_assoc_cmh_perm of libhpgv_host.so (include/hpgv_host.h): run_assoc_cmh's file at out_path and the max(T) empirical
    p-values of CHISQ_CMH under n_perms label shuffles within the strata at out_path + ".mperm".  Paths may be None.  Returns
    (variants written, cohort samples used, strata)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_cmh_perm.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_size_t,
                                          C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, used, k = C.c_long(0), C.c_long(0), C.c_int(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_cmh_perm(enc(vcf_path), enc(ped_path), enc(within_path), enc(out_path), int(n_perms), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   batch_bytes, C.byref(n), C.byref(used), C.byref(k))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_cmh_perm -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, used.value, k.value


def within_read(within_path, names, take=None):
    """hpgv_host_within_read of libhpgv_host.so: the stratum of every sample of `names` (a list of str) by the within file, -1
    without a line or where take (n,) is 0; strata numbered by first appearance among the samples taken.  Returns (stratum (n,)
    int32, n_strata).  Raises HpgvError (code ERR_INVALID) on a short or ragged line, a duplicate id, more than CMH_MAX_STRATA
    cluster names or an unreadable file."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_host_within_read.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    H.hpgv_host_last_error.restype = C.c_char_p
    arr = (C.c_char_p * max(len(names), 1))(*[os.fsencode(q) for q in names])
    stratum = np.full(max(len(names), 1), -1, np.int32)
    tk = None if take is None else _np(take, np.uint8)
    k = C.c_int(0)
    rc = H.hpgv_host_within_read(None if within_path is None else os.fsencode(within_path), arr, len(names), _ptr(tk), _ptr(stratum), C.byref(k))
    if rc != OK:
        e = HpgvError("hpgv_host_within_read -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return stratum[:len(names)].copy(), k.value


def cmh_fit(tables):
    """hpgv_cmh_fit: the stratified association of include/hpgv.h on the host.  tables: (K, 4) int32 {A1, A2, U1, U2} per stratum.
    Returns a CMH_RESULT record.  No device needed."""
    t = _np(tables, np.int32).reshape(-1, 4)
    out = np.zeros(1, CMH_RESULT)
    rc = load().hpgv_cmh_fit(_ptr(t) if len(t) else None, len(t), _ptr(out))
    if rc != OK:
        e = HpgvError("hpgv_cmh_fit -> %d" % rc)
        e.code = rc
        raise e
    return out[0]


def covar_read(covar_path, names, n_covar=0):
    """hpgv_host_covar_read of libhpgv_host.so: the covariate file's values for the samples `names` (a list of str).  Returns
    (cov (n, C) float64, have (n,) uint8: 1 where the sample has a line of finite values).  Raises HpgvError (code ERR_INVALID) on a
    duplicate id, a ragged line, more than LOGISTIC_MAX_COVAR columns in use or an unreadable file."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_host_covar_read.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    H.hpgv_host_last_error.restype = C.c_char_p
    arr = (C.c_char_p * max(len(names), 1))(*[os.fsencode(q) for q in names])
    cov = np.zeros((max(len(names), 1), LOGISTIC_MAX_COVAR), np.float64)
    have = np.zeros(max(len(names), 1), np.uint8)
    nc = C.c_int(0)
    rc = H.hpgv_host_covar_read(None if covar_path is None else os.fsencode(covar_path), arr, len(names), n_covar, C.byref(nc), _ptr(cov), _ptr(have))
    if rc != OK:
        e = HpgvError("hpgv_host_covar_read -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return cov[:len(names), :nc.value].copy(), have[:len(names)].copy()


def logistic_fit(cls, y, cov=None, max_iter=25, tol=1e-10):
    """hpgv_logistic_fit: the logistic regression of include/hpgv.h on the host, samples in index order.  cls: genotype classes
    (0, 1, 2; anything else missing), y: 1 = affected, cov (n, C) or None.  Returns (a LOGISTIC_RESULT record, coef (2, p): beta
    then se).  No device needed."""
    c, yy = _np(cls, np.uint8), _np(y, np.uint8)
    cv = np.zeros((len(c), 0), np.float64) if cov is None else _np(cov, np.float64).reshape(len(c), -1)
    nc = cv.shape[1]
    out = np.zeros(1, LOGISTIC_RESULT)
    coef = np.zeros((2, min(nc, LOGISTIC_MAX_COVAR) + 2), np.float64)
    rc = load().hpgv_logistic_fit(_ptr(c), _ptr(yy), _ptr(cv) if nc else None, len(c), nc, int(max_iter), float(tol), _ptr(out), _ptr(coef))
    if rc != OK:
        e = HpgvError("hpgv_logistic_fit -> %d" % rc)
        e.code = rc
        raise e
    return out[0], coef


def run_assoc_linear(vcf_path, ped_path, pheno_path, covar_path, out_path, n_covar=0, batch_bytes=1 << 22):
    """hpgv_run_assoc_linear of libhpgv_host.so (include/hpgv_host.h): one linear regression per variant of the trait -- the first
    value column of pheno_path, or the PED's sixth column without one -- with the first n_covar value columns of the covariate file
    (0: all of them; covar_path None: no covariates) at out_path.  Paths may be None.  Returns (variants written, cohort samples
    used)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_linear.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, used = C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_linear(enc(vcf_path), enc(ped_path), enc(pheno_path), enc(covar_path), n_covar, enc(out_path), batch_bytes, C.byref(n), C.byref(used))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_linear -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, used.value


def run_assoc_linear_perm(vcf_path, ped_path, pheno_path, covar_path, out_path, n_perms, seed, n_covar=0, batch_bytes=1 << 22):
    """hpgv_run_assoc_linear_perm of libhpgv_host.so (include/hpgv_host.h): run_assoc_linear's file at out_path and the max(T)
    empirical p-values of n_perms permutations of the reduced model's residuals at out_path + ".mperm".  Paths may be None.  Returns
    (variants written, cohort samples used)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_linear_perm.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_uint64, C.c_size_t,
                                             C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, used = C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_linear_perm(enc(vcf_path), enc(ped_path), enc(pheno_path), enc(covar_path), n_covar, enc(out_path), int(n_perms),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, batch_bytes, C.byref(n), C.byref(used))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_linear_perm -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, used.value


def linear_fit(cls, y, cov=None):
    """hpgv_linear_fit: the linear regression of include/hpgv.h on the host, samples in index order.  cls: genotype classes (0, 1,
    2; anything else missing), y: the trait, cov (n, C) or None.  Returns (a LINEAR_RESULT record, coef (2, p): beta then se).  No
    device needed."""
    c, yy = _np(cls, np.uint8), _np(y, np.float64)
    cv = np.zeros((len(c), 0), np.float64) if cov is None else _np(cov, np.float64).reshape(len(c), -1)
    nc = cv.shape[1]
    out = np.zeros(1, LINEAR_RESULT)
    coef = np.zeros((2, min(nc, LOGISTIC_MAX_COVAR) + 2), np.float64)
    rc = load().hpgv_linear_fit(_ptr(c), _ptr(yy), _ptr(cv) if nc else None, len(c), nc, _ptr(out), _ptr(coef))
    if rc != OK:
        e = HpgvError("hpgv_linear_fit -> %d" % rc)
        e.code = rc
        raise e
    return out[0], coef


def linear_perm_fit(cls, y, cov, order):
    """hpgv_linear_perm_fit: the permuted linear statistic of include/hpgv.h on the host for one row, samples in index order.  cls,
    y, cov as linear_fit takes them; order (n_perms, n): row p column j = the sample whose residual sample j takes.  Returns (t_obs,
    t_perm (n_perms,)).  No device needed."""
    c, yy = _np(cls, np.uint8), _np(y, np.float64)
    cv = np.zeros((len(c), 0), np.float64) if cov is None else _np(cov, np.float64).reshape(len(c), -1)
    nc = cv.shape[1]
    od = _np(order, np.int32).reshape(-1, len(c)) if len(c) else np.zeros((0, 0), np.int32)
    t_obs, t_perm = np.zeros(1, np.float64), np.zeros(max(len(od), 1), np.float64)
    rc = load().hpgv_linear_perm_fit(_ptr(c), _ptr(yy), _ptr(cv) if nc else None, len(c), nc, _ptr(od) if len(od) else None, len(od), _ptr(t_obs), _ptr(t_perm))
    if rc != OK:
        e = HpgvError("hpgv_linear_perm_fit -> %d" % rc)
        e.code = rc
        raise e
    return float(t_obs[0]), t_perm[:len(od)]


def linear_t_p(t, df):
    """hpgv_linear_t_p: the two-sided tail of Student's t with df degrees of freedom.  No device needed."""
    return float(load().hpgv_linear_t_p(float(t), int(df)))


def run_genome(vcf_path, out_path, min_pi_hat=0.0, batch_bytes=1 << 22):
    """hpgv_run_genome of libhpgv_host.so (include/hpgv_host.h): the sample pairs with PI_HAT >= min_pi_hat at out_path.  Paths may
    be None (the call then fails with ERR_INVALID).  Returns (records that took part, pairs written)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_genome.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, k = C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_genome(enc(vcf_path), enc(out_path), float(min_pi_hat), batch_bytes, C.byref(n), C.byref(k))
    if rc != OK:
        e = HpgvError("hpgv_run_genome -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, k.value


def run_grm(vcf_path, out_prefix, min_maf=0.01, batch_bytes=1 << 22):
    """hpgv_run_grm of libhpgv_host.so (include/hpgv_host.h): <out_prefix>.grm.bin, .grm.N.bin and .grm.id of the VCF's samples at
    hpgv_grm_frac_bits(min_maf).  Paths may be None (the call then fails with ERR_INVALID).  Returns (variants used, samples)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_grm.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, k = C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_grm(enc(vcf_path), enc(out_prefix), float(min_maf), batch_bytes, C.byref(n), C.byref(k))
    if rc != OK:
        e = HpgvError("hpgv_run_grm -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, k.value


def run_score(vcf_path, score_path, out_path, impute=True, batch_bytes=1 << 22):
    """hpgv_run_score of libhpgv_host.so (include/hpgv_host.h): the .profile of the VCF's samples for the score file's weights at
    out_path.  Paths may be None (the call then fails with ERR_INVALID).  Returns (variants used, samples, unmatched records)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_score.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, k, u = C.c_long(0), C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_score(enc(vcf_path), enc(score_path), enc(out_path), 1 if impute else 0, batch_bytes, C.byref(n), C.byref(k), C.byref(u))
    if rc != OK:
        e = HpgvError("hpgv_run_score -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, k.value, u.value


def _run_pca_result(what, H, rc, counts):
    if rc != OK:
        e = HpgvError("%s -> %d: %s" % (what, rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return tuple(c.value for c in counts)


def run_pca(vcf_path, out_prefix, min_maf=0.01, n_pcs=10, write_grm=False, batch_bytes=1 << 22):
    """hpgv_run_pca of libhpgv_host.so (include/hpgv_host.h): <out_prefix>.eigenval and .eigenvec of the VCF's GRM and, with
    write_grm, hpgv_run_grm's three files.  Returns (variants used, samples, sweeps; negative: not converged)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_pca.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]
    H.hpgv_host_last_error.restype = C.c_char_p
    n, k, it = C.c_long(0), C.c_long(0), C.c_int(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_pca(enc(vcf_path), enc(out_prefix), float(min_maf), int(n_pcs), 1 if write_grm else 0, batch_bytes, C.byref(n), C.byref(k), C.byref(it))
    return _run_pca_result("hpgv_run_pca", H, rc, (n, k, it))


def run_pca_grm(grm_prefix, out_prefix, n_pcs=10):
    """hpgv_run_pca_grm: the same solver on <grm_prefix>.grm.bin / .grm.id.  Returns (samples, sweeps; negative: not converged)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_pca_grm.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_int)]
    H.hpgv_host_last_error.restype = C.c_char_p
    k, it = C.c_long(0), C.c_int(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_pca_grm(enc(grm_prefix), enc(out_prefix), int(n_pcs), C.byref(k), C.byref(it))
    return _run_pca_result("hpgv_run_pca_grm", H, rc, (k, it))


class RunClumpOptions(C.Structure):
    """hpgv_run_clump_options_t, with PLINK's defaults"""
    _fields_ = [("p1", C.c_double), ("p2", C.c_double), ("min_r2", C.c_double), ("max_bp", C.c_int64), ("window", C.c_int)]

    def __init__(self, p1=1e-4, p2=1e-2, min_r2=0.5, max_bp=250000, window=1024):
        super().__init__(p1, p2, min_r2, max_bp, window)


def run_assoc_clump(vcf_path, ped_path, out_path, task=TASK_CHISQ, options=None, batch_bytes=1 << 22, **kw):
    """hpgv_run_assoc_clump of libhpgv_host.so (include/hpgv_host.h): hpgv_run_assoc's file at out_path and the clumps of its
    significant variants in out_path + ".clumped".  options: a RunClumpOptions (or its fields as keywords: p1, p2, min_r2, max_bp,
    window); paths may be None and options False (a NULL pointer): the call then fails with ERR_INVALID.  Returns (variants written, clumps, truncated candidates)."""
    _build.build_host_lib()
    H = C.CDLL(_build.HOSTLIB)
    H.hpgv_run_assoc_clump.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t] + [C.POINTER(C.c_long)] * 3
    H.hpgv_host_last_error.restype = C.c_char_p
    if options is None or kw:
        options = RunClumpOptions(**kw)
    n, k, t = C.c_long(0), C.c_long(0), C.c_long(0)
    enc = lambda q: None if q is None else os.fsencode(q)
    rc = H.hpgv_run_assoc_clump(enc(vcf_path), enc(ped_path), enc(out_path), task, C.byref(options) if options is not False else None,
                                batch_bytes, C.byref(n), C.byref(k), C.byref(t))
    if rc != OK:
        e = HpgvError("hpgv_run_assoc_clump -> %d: %s" % (rc, (H.hpgv_host_last_error() or b"").decode(errors="replace")))
        e.code = rc
        raise e
    return n.value, k.value, t.value


def perm_pvalues(t_obs, n_ge, t_max):
    """hpgv_perm_pvalues: (EMP1, EMP2) of every variant from its observed statistic, its count of permutations at or above
    it, and the per-permutation maxima merged over the whole scan.  No device needed."""
    t = _np(t_obs, np.float64)
    g = _np(n_ge, np.int32)
    m = _np(t_max, np.float64)
    assert t.shape == g.shape and t.ndim == 1 and m.ndim == 1
    emp1, emp2 = np.zeros(len(t), np.float64), np.zeros(len(t), np.float64)
    rc = load().hpgv_perm_pvalues(_ptr(t), len(t), _ptr(g), _ptr(m), len(m), _ptr(emp1), _ptr(emp2))
    if rc != OK:
        raise HpgvError("hpgv_perm_pvalues -> %d" % rc)
    return emp1, emp2


def ld_r2(counts6):
    """hpgv_ld_r2: r^2 of six counts {n, sa, sb, saa, sbb, sab} (needs no device); counts6 of shape (..., 6) gives (...)."""
    c = _np(counts6, np.int32)
    assert c.shape[-1] == 6
    flat = c.reshape(-1, 6)
    L = load()
    out = np.array([L.hpgv_ld_r2(_ptr(row)) for row in flat], np.float64)
    return out.reshape(c.shape[:-1])


def ibs_terms(class4):
    """hpgv_ibs_terms on rows of class counts (..., >= 3) = {n0, n1, n2[, missing]}: (used (...) bool, terms (..., 5)).  No device
    needed."""
    c = _np(class4, np.int32)
    flat = c.reshape(-1, c.shape[-1])
    L = load()
    used, terms = np.zeros(len(flat), bool), np.zeros((len(flat), 5), np.float64)
    for k, row in enumerate(flat):
        used[k] = L.hpgv_ibs_terms(int(row[0]), int(row[1]), int(row[2]), _ptr(terms[k])) != 0
    return used.reshape(c.shape[:-1]), terms.reshape(c.shape[:-1] + (5,))


def ibs_expected(class4):
    """E = {E00, E01, E02, E11, E12} of rows of class counts in file order: hpgv_ibs_terms of every row, the used rows' terms added
    sequentially, divided by their number (NaN without a used row).  A skipped row's class4 is zeros: it is not used."""
    used, terms = ibs_terms(class4)
    total = [0.0] * 5
    m = 0
    for u, t in zip(used.reshape(-1).tolist(), terms.reshape(-1, 5).tolist()):
        if u:
            m += 1
            total = [a + b for a, b in zip(total, t)]
    with np.errstate(invalid="ignore"):
        return np.array(total, np.float64) / np.float64(m)


def ibs_genome(counts, E):
    """hpgv_ibs_genome on an IBS_COUNTS array (or (..., 4) int32): (..., 5) = {Z0, Z1, Z2, PI_HAT, DST}.  No device needed."""
    c = np.ascontiguousarray(counts)
    if c.dtype == IBS_COUNTS:
        shape, flat = c.shape, c.reshape(-1)
    else:
        c = _np(counts, np.int32)
        shape, flat = c.shape[:-1], c.reshape(-1, 4)
    e = _np(E, np.float64)
    assert e.shape == (5,)
    L = load()
    out = np.zeros((len(flat), 5), np.float64)
    for k in range(len(flat)):
        L.hpgv_ibs_genome(C.c_void_p(flat[k:k + 1].ctypes.data), _ptr(e), _ptr(out[k]))
    return out.reshape(shape + (5,))


def ibs_plan_rows(n_variants, n_cols, n_cus):
    """hpgv_ibs_plan_rows: rows per row range of hpgv_ibs_pairs_dev's launch"""
    return int(load().hpgv_ibs_plan_rows(int(n_variants), int(n_cols), int(n_cus)))


def grm_table(class4, frac_bits, min_maf):
    """hpgv_grm_table on rows of class counts (..., >= 3) = {n0, n1, n2[, missing]}: (used (...) bool, table (...) GRM_TAB).  No
    device needed."""
    c = _np(class4, np.int32)
    flat = c.reshape(-1, c.shape[-1])
    L = load()
    used, tab = np.zeros(len(flat), bool), np.zeros(len(flat), GRM_TAB)
    raw = tab.view(np.int8).reshape(len(flat), 8)
    for k, row in enumerate(flat):
        used[k] = L.hpgv_grm_table(int(row[0]), int(row[1]), int(row[2]), int(frac_bits), float(min_maf), _ptr(raw[k, :4]), _ptr(raw[k, 4:])) != 0
    return used.reshape(c.shape[:-1]), tab.reshape(c.shape[:-1])


def grm_frac_bits(min_maf):
    """hpgv_grm_frac_bits: the largest frac_bits that loses no row with MAF >= min_maf, -1 for min_maf outside (0, 0.5]"""
    return int(load().hpgv_grm_frac_bits(float(min_maf)))


def grm_value(acc, frac_bits):
    """hpgv_grm_value on a GRM_ACC array (or (..., 2) int64 = {sq, n}): (...) float64.  No device needed."""
    a = np.ascontiguousarray(acc)
    if a.dtype == GRM_ACC:
        shape, flat = a.shape, a.reshape(-1)
    else:
        a = _np(acc, np.int64)
        shape, flat = a.shape[:-1], a.reshape(-1, 2)
    L = load()
    out = np.zeros(len(flat), np.float64)
    for k in range(len(flat)):
        out[k] = L.hpgv_grm_value(C.c_void_p(flat[k:k + 1].ctypes.data), int(frac_bits))
    return out.reshape(shape)


def pca_block(k):
    """hpgv_pca_block: the solver's block width for k pairs (16, 32 or -1)"""
    return int(load().hpgv_pca_block(int(k)))


def pca_jacobi(H):
    """hpgv_pca_jacobi of a symmetric (L, L) matrix: (theta (L,), W (L, L)) with W[:, j] the unit eigenvector of theta[j], the pairs
    by decreasing |theta|.  No device needed."""
    W = np.array(H, np.float64, order="C")
    L = W.shape[0]
    theta = np.zeros(L, np.float64)
    rc = load().hpgv_pca_jacobi(L, _ptr(W), _ptr(theta))
    if rc != OK:
        raise HpgvError("hpgv_pca_jacobi -> %d" % rc)
    return theta, W


def pca_chol_inv(G):
    """hpgv_pca_chol_inv of an (L, L) matrix: (failed, M) with M = R^-1 of G = R^T R; failed: a pivot fell to or below
    L * eps * max diag.  No device needed."""
    G = np.ascontiguousarray(G, np.float64)
    M = np.zeros_like(G)
    rc = load().hpgv_pca_chol_inv(G.shape[0], _ptr(G), _ptr(M))
    if rc < 0:
        raise HpgvError("hpgv_pca_chol_inv -> %d" % rc)
    return rc != 0, M


def grm_plan_rows(n_variants, n_cols, n_cus):
    """hpgv_grm_plan_rows: rows per row range of hpgv_grm_pairs_dev's launch"""
    return int(load().hpgv_grm_plan_rows(int(n_variants), int(n_cols), int(n_cus)))


def score_table(class4, w, frac_bits, flags, impute):
    """hpgv_score_table on rows of class counts (n, >= 3), weights (n, n_scores) and flag bytes (n,): (used (n,) bool, limbs
    (n, n_scores, 8) int8 = the limbs of qg then of qm, c (n, n_scores) int64).  No device needed."""
    c4 = _np(class4, np.int32)
    c4 = c4.reshape(-1, c4.shape[-1])
    wv = _np(w, np.float64).reshape(len(c4), -1)
    ns = wv.shape[1]
    s = _np(frac_bits, np.int32).reshape(-1)
    fl = _np(flags, np.uint8).reshape(-1)
    L = load()
    used, limbs, c = np.zeros(len(c4), bool), np.zeros((len(c4), ns, 8), np.int8), np.zeros((len(c4), ns), np.int64)
    for k, row in enumerate(c4):
        used[k] = L.hpgv_score_table(int(row[0]), int(row[1]), int(row[2]), _ptr(wv[k]), ns, _ptr(s), int(fl[k]), 1 if impute else 0,
                                     _ptr(limbs[k]), _ptr(c[k])) != 0
    return used, limbs, c


def score_frac_bits(max_abs_w):
    """hpgv_score_frac_bits: the largest frac_bits at which no weight at or below max_abs_w makes its row unused"""
    return int(load().hpgv_score_frac_bits(float(max_abs_w)))


def score_value(sums, cnst, frac_bits):
    """hpgv_score_value, element-wise on int64 sums with one constant: float64 of the same shape.  No device needed."""
    a = _np(sums, np.int64)
    L = load()
    out = np.zeros(a.size, np.float64)
    for k, v in enumerate(a.reshape(-1)):
        out[k] = L.hpgv_score_value(int(v), int(cnst), int(frac_bits))
    return out.reshape(a.shape)


def score_plan_rows(n_variants, n_cols, n_scores, n_cus):
    """hpgv_score_plan_rows: rows per row range of hpgv_score_cols_dev's launch"""
    return int(load().hpgv_score_plan_rows(int(n_variants), int(n_cols), int(n_scores), int(n_cus)))


def clump(p, edges, p1):
    """hpgv_clump: PLINK's default --clump on candidates with p-values p and LD edges between them (an LD_EDGE array, or an (m, 2)
    array of candidate numbers).  Returns (index_of [n]: the index candidate of each one's clump or -1, clump_order: the index
    candidates in the order the clumps were opened).  No device needed."""
    pv = _np(p, np.float64)
    e = np.asarray(edges)
    if e.dtype != LD_EDGE:
        pairs = np.asarray(edges, np.int64).reshape(-1, 2)
        e = np.zeros(len(pairs), LD_EDGE)
        e["a"], e["b"] = pairs[:, 0], pairs[:, 1]
    e = np.ascontiguousarray(e)
    index_of, order = np.zeros(len(pv), np.int32), np.zeros(len(pv), np.int32)
    k = C.c_int(0)
    rc = load().hpgv_clump(len(pv), _ptr(pv), _ptr(e), len(e), float(p1), _ptr(index_of), _ptr(order), C.byref(k))
    if rc != OK:
        err = HpgvError("hpgv_clump -> %d" % rc)
        err.code = rc
        raise err
    return index_of, order[:k.value].copy()


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _text_call(text, max_lines):
    """what a *_text wrapper opens with: the text as bytes, max_lines (default: a line per newline and one more), the length m
    of its per-line arrays (at least 1), a zeroed status [m] and the cell for n_lines"""
    if isinstance(text, str):
        text = text.encode()
    if max_lines is None:
        max_lines = text.count(b"\n") + 1
    m = max(max_lines, 1)
    return text, max_lines, m, np.zeros(m, np.int32), C.c_int(0)


def _text_result(nl, max_lines, **per_line):
    """and what it closes with: n_lines and every per-line array (None stays None) cut to the lines the call wrote,
    min(n_lines, max_lines)"""
    k = min(nl.value, max_lines)
    return dict(n_lines=nl.value, **{key: None if a is None else a[:k] for key, a in per_line.items()})


class Engine:
    """One engine context on one device (thin wrapper over hpgv_ctx)."""

    def __init__(self, device=0):
        """device: one device id, or a list of ids for a group context (hpgv_create_multi)."""
        self.L = load()
        h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (C.c_int * len(device))(*device)
            rc = self.L.hpgv_create_multi(ids, len(device), C.byref(h))
        else:
            rc = self.L.hpgv_create(device, C.byref(h))
        if rc != OK:
            raise HpgvError("hpgv_create(%s) -> %d: %s" % (device, rc, self.L.hpgv_last_error(None).decode()))
        self.h = h
        self.device = device
        self._bufs = []
        self._views = []

    def close(self):
        if getattr(self, "h", None):
            # member views of a group hold their member's raw handle: they go first (their buffers are freed while the
            # member context is alive, and their handle is cleared so that a later close()/__del__ of the view is a no-op)
            for v in getattr(self, "_views", []):
                v.close()
            self._views = []
            for b in self._bufs:
                self.L.hpgv_dev_free(self.h, b)
            self._bufs = []
            for b in getattr(self, "_host_bufs", []):
                self.L.hpgv_host_free(self.h, b)
            self._host_bufs = []
            if not getattr(self, "_view", False):
                self.L.hpgv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise HpgvError("hpgv error %d: %s" % (rc, self.L.hpgv_last_error(self.h).decode()))

    def set_option(self, key, value):
        self._chk(self.L.hpgv_set_option(self.h, key.encode(), int(value)))

    # ---- cohort -----------------------------------------------------------
    def set_cohort(self, condition):
        c = _np(condition, np.uint8)
        self._chk(self.L.hpgv_set_cohort(self.h, _ptr(c), len(c)))
        self._n_perms = 0               # a new cohort drops the label rows
        self._n_covar = 0               # and the covariates
        self._n_strata = 0              # and the strata
        self._n_samples = len(c)
        return self.assoc_layout()

    def set_perm_labels(self, labels):
        """hpgv_set_perm_labels: labels (n_perms, n_samples) of 0 / 1 in VCF column order; None or no rows drops them."""
        if labels is None or len(labels) == 0:
            self._chk(self.L.hpgv_set_perm_labels(self.h, None, 0))
            self._n_perms = 0
            return
        lab = _np(labels, np.uint8)
        assert lab.ndim == 2
        self._chk(self.L.hpgv_set_perm_labels(self.h, _ptr(lab), lab.shape[0]))
        self._n_perms = lab.shape[0]

    def assoc_layout(self):
        a, u, p = C.c_int(), C.c_int(), C.c_size_t()
        self._chk(self.L.hpgv_assoc_layout(self.h, C.byref(a), C.byref(u), C.byref(p)))
        return a.value, u.value, p.value

    def set_families(self, n_samples, father_col, mother_col, child_off, child_col, child_sex):
        f, m = _np(father_col, np.int32), _np(mother_col, np.int32)
        o, c, s = _np(child_off, np.int32), _np(child_col, np.int32), _np(child_sex, np.uint8)
        assert len(o) == len(f) + 1 and len(c) == len(s)
        self._chk(self.L.hpgv_set_families(self.h, n_samples, len(f), _ptr(f), _ptr(m), _ptr(o),
                                           _ptr(c), _ptr(s)))
        self._n_flips = 0               # new families drop the flip rows
        self._n_families = len(f)
        return self.tdt_layout()

    def set_tdt_flips(self, flips):
        """hpgv_set_tdt_flips: flips (n_perms, n_families) of 0 / 1 (1 = flipped) by the family index of set_families; None or no
        rows drops them."""
        if flips is None or len(flips) == 0:
            self._chk(self.L.hpgv_set_tdt_flips(self.h, None, 0))
            self._n_flips = 0
            return
        fl = _np(flips, np.uint8)
        assert fl.ndim == 2 and fl.shape[1] == getattr(self, "_n_families", fl.shape[1])
        self._chk(self.L.hpgv_set_tdt_flips(self.h, _ptr(fl), fl.shape[0]))
        self._n_flips = fl.shape[0]

    def tdt_layout(self):
        a, b, p = C.c_int(), C.c_int(), C.c_size_t()
        self._chk(self.L.hpgv_tdt_layout(self.h, C.byref(a), C.byref(b), C.byref(p)))
        return a.value, b.value, p.value

    def set_logfact(self, table):
        t = _np(table, np.float64)
        self._chk(self.L.hpgv_set_logfact(self.h, _ptr(t), len(t)))

    def set_stats_cohort(self, n_samples):
        self._chk(self.L.hpgv_set_stats_cohort(self.h, n_samples))
        p = C.c_size_t()
        self._chk(self.L.hpgv_stats_layout(self.h, C.byref(p)))
        return p.value

    def set_stats_groups(self, group_of_sample, n_groups):
        g = _np(group_of_sample, np.int32)
        self._chk(self.L.hpgv_set_stats_groups(self.h, _ptr(g), len(g), n_groups))
        p = C.c_size_t()
        sizes = np.zeros(n_groups, np.int32)
        self._chk(self.L.hpgv_stats_groups_layout(self.h, C.byref(p), _ptr(sizes)))
        return p.value, sizes

    def stats_scan_group(self, d_gt, n_variants, group, d_counts8, stream=None):
        self._chk(self.L.hpgv_stats_scan_group_dev(self.h, d_gt, n_variants, group, d_counts8, stream))

    def set_pedigree(self, n_samples, father_col, mother_col, child_col, child_sex):
        f, m, c = _np(father_col, np.int32), _np(mother_col, np.int32), _np(child_col, np.int32)
        s = _np(child_sex, np.uint8)
        self._chk(self.L.hpgv_set_pedigree(self.h, n_samples, len(c), _ptr(f), _ptr(m), _ptr(c), _ptr(s)))
        p = C.c_size_t()
        self._chk(self.L.hpgv_mendel_layout(self.h, C.byref(p)))
        return p.value

    def set_text_inheritance_filters(self, min_dominant=-1.0, min_recessive=-1.0):
        """--inh-dom / --inh-rec of the *_text entry points (negative: off)"""
        self._chk(self.L.hpgv_set_text_inheritance_filters(self.h, min_dominant, min_recessive))

    def mendel_scan(self, d_gt, n_variants, d_errors, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_mendel_scan_dev(self.h, d_gt, n_variants, d_is_x, d_errors, stream))

    def mendel_children(self, d_gt, n_variants, d_child_errors, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_mendel_children_dev(self.h, d_gt, n_variants, d_is_x, d_child_errors, stream))

    # ---- device memory ------------------------------------------------------
    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.L.hpgv_dev_alloc(self.h, nbytes, C.byref(p)))
        self._bufs.append(p)
        return p

    def free(self, p):
        self._bufs = [b for b in self._bufs if b.value != p.value]
        self._chk(self.L.hpgv_dev_free(self.h, p))

    def host_array(self, shape, dtype=np.uint8):
        """numpy array in page-locked host memory (hpgv_host_alloc): batches staged into it are read by the
        per-batch kernels in place, without a copy.  Freed with the engine."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self.L.hpgv_host_alloc(self.h, max(n, 16), C.byref(p)))
        self._host_bufs = getattr(self, "_host_bufs", []) + [p]
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.hpgv_memcpy_h2d(self.h, dptr, _ptr(arr), arr.nbytes, None))

    def d2h(self, dptr, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._chk(self.L.hpgv_memcpy_d2h(self.h, _ptr(out), dptr, out.nbytes, None))
        return out

    def sync(self, stream=None):
        self._chk(self.L.hpgv_stream_sync(self.h, stream))

    # ---- per-batch host entry points ---------------------------------------
    def assoc(self, task, gt, is_x=None):
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        A1, A2, U1, U2 = (np.zeros(nv, np.int32) for _ in range(4))
        odds, chisq, p = (np.zeros(nv, np.float64) for _ in range(3))
        self._chk(self.L.hpgv_assoc(self.h, task, _ptr(gt), pitch, nv, _ptr(x), _ptr(A1), _ptr(A2),
                                    _ptr(U1), _ptr(U2), _ptr(odds),
                                    _ptr(chisq) if task == TASK_CHISQ else None, _ptr(p)))
        return dict(A1=A1, A2=A2, U1=U1, U2=U2, odds=odds,
                    chisq=chisq if task == TASK_CHISQ else None, p=p)

    def assoc_perm(self, gt, is_x=None):
        """hpgv_assoc_perm: hpgv_assoc with task CHISQ plus n_ge per variant and batch_max per permutation."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        A1, A2, U1, U2, n_ge = (np.zeros(nv, np.int32) for _ in range(5))
        odds, chisq, p = (np.zeros(nv, np.float64) for _ in range(3))
        bmax = np.zeros(max(getattr(self, "_n_perms", 0), 1), np.float64)
        self._chk(self.L.hpgv_assoc_perm(self.h, _ptr(gt), pitch, nv, _ptr(x), _ptr(A1), _ptr(A2), _ptr(U1), _ptr(U2),
                                         _ptr(odds), _ptr(chisq), _ptr(p), _ptr(n_ge), _ptr(bmax)))
        return dict(A1=A1, A2=A2, U1=U1, U2=U2, odds=odds, chisq=chisq, p=p, n_ge=n_ge, batch_max=bmax[:self._n_perms])

    def assoc_perm_text(self, text, max_lines=None):
        """hpgv_assoc_perm_text: hpgv_assoc_text with task CHISQ plus n_ge per line and batch_max per permutation."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        A1, A2, U1, U2, n_ge = (np.zeros(m, np.int32) for _ in range(5))
        odds, chisq, p = (np.zeros(m, np.float64) for _ in range(3))
        bmax = np.zeros(max(getattr(self, "_n_perms", 0), 1), np.float64)
        self._chk(self.L.hpgv_assoc_perm_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                              _ptr(A1), _ptr(A2), _ptr(U1), _ptr(U2), _ptr(odds), _ptr(chisq), _ptr(p),
                                              _ptr(n_ge), _ptr(bmax)))
        return dict(_text_result(nl, max_lines, status=status, A1=A1, A2=A2, U1=U1, U2=U2, odds=odds, chisq=chisq, p=p, n_ge=n_ge),
                    batch_max=bmax[:self._n_perms])

    def assoc_model(self, gt, perm=False):
        """hpgv_assoc_model: counts8 (nv, 8), chisq5 and p5 (nv, 5; columns MODEL_*); perm=True adds the trend permutation's n_ge
        per variant and batch_max per permutation of the labels set with set_perm_labels."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        c8 = np.zeros((nv, 8), np.int32)
        chisq5, p5 = np.zeros((nv, 5), np.float64), np.zeros((nv, 5), np.float64)
        np_ = getattr(self, "_n_perms", 0)
        n_ge, bmax = (np.zeros(nv, np.int32), np.zeros(max(np_, 1), np.float64)) if perm else (None, None)
        self._chk(self.L.hpgv_assoc_model(self.h, _ptr(gt), pitch, nv, _ptr(c8), _ptr(chisq5), _ptr(p5), _ptr(n_ge), _ptr(bmax)))
        res = dict(counts8=c8, chisq5=chisq5, p5=p5)
        if perm:
            res.update(n_ge=n_ge, batch_max=bmax[:np_])
        return res

    def assoc_model_text(self, text, max_lines=None, perm=False):
        """hpgv_assoc_model_text: assoc_model on VCF data lines, the outputs per line; perm as in assoc_model."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        c8 = np.zeros((m, 8), np.int32)
        chisq5, p5 = np.zeros((m, 5), np.float64), np.zeros((m, 5), np.float64)
        np_ = getattr(self, "_n_perms", 0)
        n_ge, bmax = (np.zeros(m, np.int32), np.zeros(max(np_, 1), np.float64)) if perm else (None, None)
        self._chk(self.L.hpgv_assoc_model_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                               _ptr(c8), _ptr(chisq5), _ptr(p5), _ptr(n_ge), _ptr(bmax)))
        if not perm:
            return _text_result(nl, max_lines, status=status, counts8=c8, chisq5=chisq5, p5=p5)
        return dict(_text_result(nl, max_lines, status=status, counts8=c8, chisq5=chisq5, p5=p5, n_ge=n_ge), batch_max=bmax[:np_])

    def set_strata(self, stratum, n_strata=None):
        """hpgv_set_strata: stratum (n_samples,) int32 in VCF column order, negative = in no stratum; n_strata defaults to the largest
        value + 1.  None, or n_strata 0, drops the strata."""
        if stratum is None or n_strata == 0:
            self._chk(self.L.hpgv_set_strata(self.h, None, 0, 0))
            self._n_strata = 0
            return
        st = _np(stratum, np.int32)
        k = int(st.max()) + 1 if n_strata is None else int(n_strata)
        self._chk(self.L.hpgv_set_strata(self.h, _ptr(st), len(st), k))
        self._n_strata = k

    def assoc_cmh(self, gt, is_x=None, tables=False):
        """hpgv_assoc_cmh: a CMH_RESULT array (nv,) and, with tables, (nv, K, 4) int32 {A1, A2, U1, U2} per stratum."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        out = np.zeros(nv, CMH_RESULT)
        tb = np.zeros((nv, getattr(self, "_n_strata", 0), 4), np.int32) if tables else None
        self._chk(self.L.hpgv_assoc_cmh(self.h, _ptr(gt), pitch, nv, _ptr(x), _ptr(out), _ptr(tb)))
        return (out, tb) if tables else out

    def assoc_cmh_text(self, text, max_lines=None, tables=False, out=None):
        """hpgv_assoc_cmh_text: assoc_cmh on VCF data lines, the outputs per line.  out: a CMH_RESULT array to write into (the
        records of skipped lines stay as they are)."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        if out is None:
            out = np.zeros(m, CMH_RESULT)
        assert out.dtype == CMH_RESULT and len(out) >= m and out.flags.c_contiguous
        tb = np.zeros((m, getattr(self, "_n_strata", 0), 4), np.int32) if tables else None
        self._chk(self.L.hpgv_assoc_cmh_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), _ptr(out), _ptr(tb)))
        return _text_result(nl, max_lines, status=status, out=out, tables=tb)

    def assoc_cmh_perm(self, gt, is_x=None):
        """hpgv_assoc_cmh_perm: assoc_cmh's records plus the permutation within strata of the labels set with set_perm_labels: a
        dict of out (CMH_RESULT (nv,)), n_ge per variant and batch_max per permutation."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        out, n_ge = np.zeros(nv, CMH_RESULT), np.zeros(nv, np.int32)
        np_ = getattr(self, "_n_perms", 0)
        bmax = np.zeros(max(np_, 1), np.float64)
        self._chk(self.L.hpgv_assoc_cmh_perm(self.h, _ptr(gt), pitch, nv, _ptr(x), _ptr(out), _ptr(n_ge), _ptr(bmax)))
        return dict(out=out, n_ge=n_ge, batch_max=bmax[:np_])

    def assoc_cmh_perm_text(self, text, max_lines=None, out=None):
        """hpgv_assoc_cmh_perm_text: assoc_cmh_perm on VCF data lines, out and n_ge per line.  out: a CMH_RESULT array to write into
        (the records of skipped lines stay as they are)."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        if out is None:
            out = np.zeros(m, CMH_RESULT)
        assert out.dtype == CMH_RESULT and len(out) >= m and out.flags.c_contiguous
        n_ge = np.zeros(m, np.int32)
        np_ = getattr(self, "_n_perms", 0)
        bmax = np.zeros(max(np_, 1), np.float64)
        self._chk(self.L.hpgv_assoc_cmh_perm_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), _ptr(out),
                                                  _ptr(n_ge), _ptr(bmax)))
        return dict(_text_result(nl, max_lines, status=status, out=out, n_ge=n_ge), batch_max=bmax[:np_])

    def set_covariates(self, cov):
        """hpgv_set_covariates: cov (n_samples, C) in VCF column order; None or no columns clears them."""
        if cov is None or np.asarray(cov).size == 0:
            self._chk(self.L.hpgv_set_covariates(self.h, None, getattr(self, "_n_samples", 0), 0))
            self._n_covar = 0
            return
        cv = _np(cov, np.float64)
        assert cv.ndim == 2
        self._chk(self.L.hpgv_set_covariates(self.h, _ptr(cv), cv.shape[0], cv.shape[1]))
        self._n_covar = cv.shape[1]

    def assoc_logistic(self, gt, max_iter=25, tol=1e-10, coef=False):
        """hpgv_assoc_logistic: a LOGISTIC_RESULT array (nv,) and, with coef, (nv, 2, p): beta then se of every coefficient."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        out = np.zeros(nv, LOGISTIC_RESULT)
        cf = np.zeros((nv, 2, getattr(self, "_n_covar", 0) + 2), np.float64) if coef else None
        self._chk(self.L.hpgv_assoc_logistic(self.h, _ptr(gt), pitch, nv, int(max_iter), float(tol), _ptr(out), _ptr(cf)))
        return (out, cf) if coef else out

    def assoc_logistic_text(self, text, max_lines=None, max_iter=25, tol=1e-10, coef=False):
        """hpgv_assoc_logistic_text: assoc_logistic on VCF data lines, the outputs per line."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        out = np.zeros(m, LOGISTIC_RESULT)
        cf = np.zeros((m, 2, getattr(self, "_n_covar", 0) + 2), np.float64) if coef else None
        self._chk(self.L.hpgv_assoc_logistic_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                                  int(max_iter), float(tol), _ptr(out), _ptr(cf)))
        return _text_result(nl, max_lines, status=status, out=out, coef=cf)

    def set_phenotype(self, y):
        """hpgv_set_phenotype: y (n_samples,) in VCF column order; None clears it."""
        if y is None:
            self._chk(self.L.hpgv_set_phenotype(self.h, None, 0))
            return
        yy = _np(y, np.float64)
        self._chk(self.L.hpgv_set_phenotype(self.h, _ptr(yy), len(yy)))

    def assoc_linear(self, gt, coef=False):
        """hpgv_assoc_linear: a LINEAR_RESULT array (nv,) and, with coef, (nv, 2, p): beta then se of every coefficient."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        out = np.zeros(nv, LINEAR_RESULT)
        cf = np.zeros((nv, 2, getattr(self, "_n_covar", 0) + 2), np.float64) if coef else None
        self._chk(self.L.hpgv_assoc_linear(self.h, _ptr(gt), pitch, nv, _ptr(out), _ptr(cf)))
        return (out, cf) if coef else out

    def assoc_linear_text(self, text, max_lines=None, coef=False):
        """hpgv_assoc_linear_text: assoc_linear on VCF data lines, the outputs per line."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        out = np.zeros(m, LINEAR_RESULT)
        cf = np.zeros((m, 2, getattr(self, "_n_covar", 0) + 2), np.float64) if coef else None
        self._chk(self.L.hpgv_assoc_linear_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), _ptr(out), _ptr(cf)))
        return _text_result(nl, max_lines, status=status, out=out, coef=cf)

    def set_linear_perms(self, order):
        """hpgv_set_linear_perms: order (n_perms, n_samples) int32 as perm_order_shuffle writes it; None or no rows drops them."""
        if order is None or len(order) == 0:
            self._chk(self.L.hpgv_set_linear_perms(self.h, None, 0))
            self._n_linperms = 0
            return
        od = _np(order, np.int32)
        assert od.ndim == 2
        self._n_linperms = 0
        self._chk(self.L.hpgv_set_linear_perms(self.h, _ptr(od), od.shape[0]))
        self._n_linperms = od.shape[0]

    def assoc_linear_perm(self, gt):
        """hpgv_assoc_linear_perm: the LINEAR_RESULT records of assoc_linear plus t_obs and n_ge per variant and batch_max per
        permutation."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        np_ = getattr(self, "_n_linperms", 0)
        out, t_obs, n_ge = np.zeros(nv, LINEAR_RESULT), np.zeros(nv, np.float64), np.zeros(nv, np.int32)
        bmax = np.zeros(max(np_, 1), np.float64)
        self._chk(self.L.hpgv_assoc_linear_perm(self.h, _ptr(gt), pitch, nv, _ptr(out), _ptr(t_obs), _ptr(n_ge), _ptr(bmax)))
        return dict(out=out, t_obs=t_obs, n_ge=n_ge, batch_max=bmax[:np_])

    def assoc_linear_perm_text(self, text, max_lines=None):
        """hpgv_assoc_linear_perm_text: assoc_linear_perm on VCF data lines, the outputs per line."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        np_ = getattr(self, "_n_linperms", 0)
        out, t_obs, n_ge = np.zeros(m, LINEAR_RESULT), np.zeros(m, np.float64), np.zeros(m, np.int32)
        bmax = np.zeros(max(np_, 1), np.float64)
        self._chk(self.L.hpgv_assoc_linear_perm_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), _ptr(out), _ptr(t_obs),
                                                     _ptr(n_ge), _ptr(bmax)))
        return dict(_text_result(nl, max_lines, status=status, out=out, t_obs=t_obs, n_ge=n_ge), batch_max=bmax[:np_])

    def ld(self, gt, window, chrom=None, pos=None, max_bp=-1, counts=True):
        """hpgv_ld: r2 (nv, window) and, with counts, counts6 (nv, window, 6); element [b, d - 1] is the pair (b - d, b) over the
        cohort columns.  chrom / pos (per row, both or neither) and max_bp bound the band."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        ch = None if chrom is None else _np(chrom, np.int32)
        po = None if pos is None else _np(pos, np.uint32)
        r2 = np.zeros((nv, window), np.float64)
        c6 = np.zeros((nv, window, 6), np.int32) if counts else None
        self._chk(self.L.hpgv_ld(self.h, _ptr(gt), pitch, nv, window, _ptr(ch), _ptr(po), int(max_bp), _ptr(r2), _ptr(c6)))
        return dict(r2=r2, counts6=c6)

    def ld_edges(self, gt, window, min_r2, chrom=None, pos=None, max_bp=-1, edge_cap=None):
        """hpgv_ld_edges: the pairs of hpgv_ld's band with r2 >= min_r2 as an LD_EDGE array sorted by (b, a).  Without edge_cap the
        call is repeated once with room when the first list was too short; with it, (edges or None, n_edges) comes back as is."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        ch = None if chrom is None else _np(chrom, np.int32)
        po = None if pos is None else _np(pos, np.uint32)
        n = C.c_uint64(0)
        cap = 4096 if edge_cap is None else int(edge_cap)
        for _ in range(2):
            e = np.zeros(max(cap, 1), LD_EDGE)
            self._chk(self.L.hpgv_ld_edges(self.h, _ptr(gt), pitch, nv, window, _ptr(ch), _ptr(po), int(max_bp), float(min_r2),
                                           _ptr(e), cap, C.byref(n)))
            if edge_cap is not None:
                return (e[:n.value] if n.value <= cap else None), n.value
            if n.value <= cap:
                return e[:n.value]
            cap = n.value
        raise HpgvError("hpgv_ld_edges: the count grew between two calls on the same rows")

    def ld_text(self, text, window, max_lines=None, counts=True):
        """hpgv_ld_text: ld on VCF data lines, one row of the window per line (skipped lines keep their slot)."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        r2 = np.zeros((m, max(window, 1)), np.float64)
        c6 = np.zeros((m, max(window, 1), 6), np.int32) if counts else None
        self._chk(self.L.hpgv_ld_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), window, _ptr(r2), _ptr(c6)))
        return _text_result(nl, max_lines, status=status, r2=r2, counts6=c6)

    def ibs(self, gt, d_counts, skip=None):
        """hpgv_ibs: class4 (nv, 4) of the rows; their pair counts are ADDED to the device records d_counts (n_samples x n_samples
        IBS_COUNTS, zeroed by the caller: memset_dev)."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        sk = None if skip is None else _np(skip, np.uint8)
        class4 = np.zeros((nv, 4), np.int32)
        self._chk(self.L.hpgv_ibs(self.h, _ptr(gt), pitch, nv, _ptr(sk), _ptr(class4), d_counts))
        return class4

    def ibs_text(self, text, d_counts, max_lines=None):
        """hpgv_ibs_text: ibs on VCF data lines (dropped lines and chromosome-X lines are skipped rows): status and class4 per line."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        class4 = np.zeros((m, 4), np.int32)
        self._chk(self.L.hpgv_ibs_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), _ptr(class4), d_counts))
        return _text_result(nl, max_lines, status=status, class4=class4)

    def grm(self, gt, d_acc, frac_bits, min_maf, skip=None):
        """hpgv_grm: class4 (nv, 4) of the rows; their pair sums are ADDED to the device records d_acc (n_samples x n_samples
        GRM_ACC, zeroed by the caller: memset_dev)."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        sk = None if skip is None else _np(skip, np.uint8)
        class4 = np.zeros((nv, 4), np.int32)
        self._chk(self.L.hpgv_grm(self.h, _ptr(gt), pitch, nv, _ptr(sk), int(frac_bits), float(min_maf), _ptr(class4), d_acc))
        return class4

    def grm_text(self, text, d_acc, frac_bits, min_maf, max_lines=None):
        """hpgv_grm_text: grm on VCF data lines (dropped lines and chromosome-X lines are skipped rows): status and class4 per line."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        class4 = np.zeros((m, 4), np.int32)
        self._chk(self.L.hpgv_grm_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), int(frac_bits), float(min_maf),
                                       _ptr(class4), d_acc))
        return _text_result(nl, max_lines, status=status, class4=class4)

    def score(self, gt, w, flags, frac_bits, impute, d_acc, acc_pitch, d_const):
        """hpgv_score: class4 (nv, 4) of the rows; their sums are ADDED to the device arrays d_acc ((n_scores + 2) x acc_pitch
        int64) and d_const (n_scores + 1 int64), both zeroed by the caller: memset_dev."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        wv = _np(w, np.float64).reshape(nv, -1)
        s = _np(frac_bits, np.int32).reshape(-1)
        fl = _np(flags, np.uint8).reshape(-1)
        class4 = np.zeros((nv, 4), np.int32)
        self._chk(self.L.hpgv_score(self.h, _ptr(gt), pitch, nv, _ptr(wv), _ptr(fl), len(s), _ptr(s), 1 if impute else 0, _ptr(class4), d_acc, acc_pitch,
                                    d_const))
        return class4

    def score_text(self, text, weigh, n_scores, frac_bits, impute, d_acc, acc_pitch, d_const, max_lines=None):
        """hpgv_score_text: score on VCF data lines.  weigh(text, n_lines, line_off, field_off, status, w, flags) is called once with
        numpy views -- line_off (n_lines + 1,), field_off (n_lines, 10), status (n_lines,), and w (n_lines, n_scores) and flags
        (n_lines,) to fill -- and returns 0 (or None) to go on.  status and class4 per line come back."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        class4 = np.zeros((m, 4), np.int32)
        s = _np(frac_bits, np.int32).reshape(-1)

        def thunk(_user, _text, n, line_off, field_off, st, w, flags):
            arr = np.ctypeslib.as_array
            rc = weigh(text, n, arr(line_off, (n + 1,)), arr(field_off, (n, 10)), arr(st, (n,)), arr(w, (n, int(n_scores))), arr(flags, (n,)))
            return int(rc or 0)

        cb = SCORE_WEIGH_FN(thunk)
        self._chk(self.L.hpgv_score_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status), cb, None, int(n_scores), _ptr(s),
                                         1 if impute else 0, _ptr(class4), d_acc, acc_pitch, d_const))
        return _text_result(nl, max_lines, status=status, class4=class4)

    def ibs_select(self, d_counts, n_cols, E, min_pi_hat, cap=None):
        """hpgv_ibs_select_dev on device records: the pairs with PI_HAT >= min_pi_hat as an IBS_PAIR array sorted by (i, j).  Without
        cap the call is repeated once with room when the first list was too short; with it, (pairs or None, count) comes back."""
        e = _np(E, np.float64)
        room = 4096 if cap is None else int(cap)
        d_n = self.alloc(16)
        try:
            for _ in range(2):
                d_pairs = self.alloc(max(room, 1) * 32)
                try:
                    self.ibs_select_dev(d_counts, n_cols, e, min_pi_hat, d_pairs if room else None, room, d_n)
                    self.sync()
                    n = int(self.d2h(d_n, (1,), np.uint64)[0])
                    pairs = self.d2h(d_pairs, (min(n, room),), IBS_PAIR) if min(n, room) else np.zeros(0, IBS_PAIR)
                finally:
                    self.free(d_pairs)
                pairs = pairs[np.lexsort((pairs["j"], pairs["i"]))]
                if cap is not None:
                    return (pairs if n <= room else None), n
                if n <= room:
                    return pairs
                room = n
        finally:
            self.free(d_n)
        raise HpgvError("hpgv_ibs_select_dev: the count grew between two calls on the same records")

    def assoc_view(self, task, gt2d, n_samples, is_x=None):
        """hpgv_assoc on a 2-D uint8 VIEW as it lies in memory (row stride = pitch): nothing is copied on the way,
        so a view of page-locked memory (host_array) is read by the kernel in place."""
        nv, pitch = gt2d.shape[0], gt2d.strides[0]
        assert gt2d.dtype == np.uint8 and gt2d.strides[1] == 1 and pitch >= n_samples
        A1, A2, U1, U2 = (np.zeros(nv, np.int32) for _ in range(4))
        odds, chisq, p = (np.zeros(nv, np.float64) for _ in range(3))
        self._chk(self.L.hpgv_assoc(self.h, task, C.c_void_p(gt2d.ctypes.data), pitch, nv,
                                    None if is_x is None else C.c_void_p(is_x.ctypes.data), _ptr(A1), _ptr(A2),
                                    _ptr(U1), _ptr(U2), _ptr(odds), _ptr(chisq) if task == TASK_CHISQ else None, _ptr(p)))
        return dict(A1=A1, A2=A2, U1=U1, U2=U2, odds=odds, chisq=chisq if task == TASK_CHISQ else None, p=p)

    def tdt_view(self, gt2d, n_samples, is_x=None):
        nv, pitch = gt2d.shape[0], gt2d.strides[0]
        assert gt2d.dtype == np.uint8 and gt2d.strides[1] == 1 and pitch >= n_samples
        t1, t2 = np.zeros(nv, np.int32), np.zeros(nv, np.int32)
        odds, chisq, p = (np.zeros(nv, np.float64) for _ in range(3))
        self._chk(self.L.hpgv_tdt(self.h, C.c_void_p(gt2d.ctypes.data), pitch, nv,
                                  None if is_x is None else C.c_void_p(is_x.ctypes.data), _ptr(t1), _ptr(t2),
                                  _ptr(odds), _ptr(chisq), _ptr(p)))
        return dict(t1=t1, t2=t2, odds=odds, chisq=chisq, p=p)

    def tdt(self, gt, is_x=None):
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        t1, t2 = np.zeros(nv, np.int32), np.zeros(nv, np.int32)
        odds, chisq, p = (np.zeros(nv, np.float64) for _ in range(3))
        self._chk(self.L.hpgv_tdt(self.h, _ptr(gt), pitch, nv, _ptr(x), _ptr(t1), _ptr(t2),
                                  _ptr(odds), _ptr(chisq), _ptr(p)))
        return dict(t1=t1, t2=t2, odds=odds, chisq=chisq, p=p)

    def tdt_perm(self, gt, is_x=None):
        """hpgv_tdt_perm: hpgv_tdt plus n_ge per variant and batch_max per permutation of the flips set with set_tdt_flips."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        t1, t2, n_ge = (np.zeros(nv, np.int32) for _ in range(3))
        odds, chisq, p = (np.zeros(nv, np.float64) for _ in range(3))
        np_ = getattr(self, "_n_flips", 0)
        bmax = np.zeros(max(np_, 1), np.float64)
        self._chk(self.L.hpgv_tdt_perm(self.h, _ptr(gt), pitch, nv, _ptr(x), _ptr(t1), _ptr(t2),
                                       _ptr(odds), _ptr(chisq), _ptr(p), _ptr(n_ge), _ptr(bmax)))
        return dict(t1=t1, t2=t2, odds=odds, chisq=chisq, p=p, n_ge=n_ge, batch_max=bmax[:np_])

    def stats(self, gt):
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        c8 = np.zeros((nv, 8), np.int32)
        chi2, p = np.zeros(nv, np.float64), np.zeros(nv, np.float64)
        self._chk(self.L.hpgv_stats(self.h, _ptr(gt), pitch, nv, _ptr(c8), _ptr(chi2), _ptr(p)))
        return dict(counts8=c8, hwe_chi2=chi2, hwe_p=p)

    def stats_groups(self, gt, n_groups):
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        c8 = np.zeros((n_groups, nv, 8), np.int32)
        chi2, p = np.zeros((n_groups, nv), np.float64), np.zeros((n_groups, nv), np.float64)
        self._chk(self.L.hpgv_stats_groups(self.h, _ptr(gt), pitch, nv, _ptr(c8), _ptr(chi2), _ptr(p)))
        return dict(counts8=c8, hwe_chi2=chi2, hwe_p=p)

    # ---- epistasis / MDR ------------------------------------------------------
    def epi_set_dataset(self, genotypes, n_affected, n_unaffected):
        d = _np(genotypes, np.uint8)
        assert d.ndim == 2 and d.shape[1] == n_affected + n_unaffected
        self._chk(self.L.hpgv_epi_set_dataset(self.h, _ptr(d), d.shape[0], n_affected, n_unaffected))
        self._epi = (d.shape[0], n_affected, n_unaffected, 1)

    def epi_set_folds(self, fold_of_sample, num_folds):
        f = _np(fold_of_sample, np.int32)
        self._chk(self.L.hpgv_epi_set_folds(self.h, _ptr(f), num_folds))
        self._epi = self._epi[:3] + (num_folds,)

    def epi_set_fold_masks(self, padded_masks, num_folds):
        m = _np(padded_masks, np.uint8)
        self._chk(self.L.hpgv_epi_set_fold_masks(self.h, _ptr(m), num_folds))
        self._epi = self._epi[:3] + (num_folds,)

    def epi_counts(self, combs, all_folds=False):
        c = _np(combs, np.int32)
        n, order = c.shape
        cells, k = 3 ** order, self._epi[3]
        shape = (k, n, cells) if all_folds else (n, cells)
        aff, unaff = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        fn = self.L.hpgv_epi_counts_all_folds if all_folds else self.L.hpgv_epi_counts
        self._chk(fn(self.h, order, _ptr(c), n, _ptr(aff), _ptr(unaff)))
        return aff, unaff

    def epi_scan_pairs(self, subset, i_begin=0, i_end=None):
        i_end = self._epi[0] if i_end is None else i_end
        n = C.c_ulonglong(0)
        self._chk(self.L.hpgv_epi_scan_pairs(self.h, i_begin, i_end, subset, None, None, C.byref(n)))
        k = self._epi[3]
        acc, mask = np.zeros((k, n.value), np.float64), np.zeros((k, n.value), np.uint16)
        if n.value:
            self._chk(self.L.hpgv_epi_scan_pairs(self.h, i_begin, i_end, subset, _ptr(acc), _ptr(mask), C.byref(n)))
        return acc, mask

    def epi_rank_pairs(self, subset, max_ranking_size, rows=None):
        k, n = self._epi[3], max_ranking_size
        ci, cj = np.zeros((k, n), np.int32), np.zeros((k, n), np.int32)
        acc, mask, cnt = np.zeros((k, n), np.float64), np.zeros((k, n), np.uint32), np.zeros(k, np.int32)
        ms = C.c_float(0)
        lo, hi = (0, self._epi[0]) if rows is None else rows
        self._chk(self.L.hpgv_epi_rank_pairs_rows(self.h, lo, hi, subset, n, _ptr(ci), _ptr(cj), _ptr(acc), _ptr(mask), _ptr(cnt),
                                                  C.byref(ms)))
        return dict(i=ci, j=cj, accuracy=acc, risky=mask, n=cnt, scan_ms=ms.value)

    def epi_scan_triples(self, subset):
        v, k = self._epi[0], self._epi[3]
        acc, mask = np.zeros((k, v, v, v), np.float64), np.zeros((k, v, v, v), np.uint32)
        self._chk(self.L.hpgv_epi_scan_triples(self.h, subset, _ptr(acc), _ptr(mask)))
        return acc, mask

    def epi_rank_triples(self, subset, max_ranking_size, rows=None):
        k, n = self._epi[3], max_ranking_size
        ci, cj, ck = (np.zeros((k, n), np.int32) for _ in range(3))
        acc, mask, cnt = np.zeros((k, n), np.float64), np.zeros((k, n), np.uint32), np.zeros(k, np.int32)
        ms = C.c_float(0)
        lo, hi = (0, self._epi[0]) if rows is None else rows
        self._chk(self.L.hpgv_epi_rank_triples_rows(self.h, lo, hi, subset, n, _ptr(ci), _ptr(cj), _ptr(ck), _ptr(acc), _ptr(mask), _ptr(cnt),
                                                    C.byref(ms)))
        return dict(i=ci, j=cj, k=ck, accuracy=acc, risky=mask, n=cnt, scan_ms=ms.value)

    def epi_eval_combs(self, combs, subset):
        """the MDR model of listed combinations of any order 2 .. 5: accuracy (n, folds), risky masks (n, folds, 8) u32"""
        c = _np(combs, np.int32)
        n, order = c.shape
        k = self._epi[3]
        acc, mask = np.zeros((n, k), np.float64), np.zeros((n, k, 8), np.uint32)
        self._chk(self.L.hpgv_epi_eval_combs(self.h, order, _ptr(c), n, subset, _ptr(acc), _ptr(mask)))
        return acc, mask

    def epi_rank_order(self, order, subset, max_ranking_size, rows=None):
        k, n = self._epi[3], max_ranking_size
        combs = np.zeros((k, n, order), np.int32)
        acc, mask, cnt = np.zeros((k, n), np.float64), np.zeros((k, n, 8), np.uint32), np.zeros(k, np.int32)
        ms = C.c_float(0)
        lo, hi = (0, self._epi[0]) if rows is None else rows
        self._chk(self.L.hpgv_epi_rank_order_rows(self.h, order, lo, hi, subset, n, _ptr(combs), _ptr(acc), _ptr(mask), _ptr(cnt), C.byref(ms)))
        return dict(combs=combs, accuracy=acc, risky=mask, n=cnt, scan_ms=ms.value)

    def epi_last_rank_info(self):
        """what the last epi_rank_pairs / _triples / _order call ran: kernel (EPI_KERNEL_*), scan launches, and the launches
        that were repeated because a candidate list overflowed"""
        info = EpiRankInfo()
        self._chk(self.L.hpgv_epi_last_rank_info(self.h, C.byref(info)))
        return dict(kernel=info.kernel, kernel_name=EPI_KERNEL_NAMES.get(info.kernel, "?"), launches=info.launches,
                    relaunches=info.relaunches)

    def epi_dataset(self, gt):
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        nA, nU, _ = self.assoc_layout()
        out = np.zeros((nv, nA + nU), np.uint8)
        self._chk(self.L.hpgv_epi_dataset(self.h, _ptr(gt), pitch, nv, _ptr(out)))
        return out

    def mendel(self, gt, is_x=None, child_errors=None):
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        x = None if is_x is None else _np(is_x, np.uint8)
        err = np.zeros(nv, np.int32)
        self._chk(self.L.hpgv_mendel(self.h, _ptr(gt), pitch, nv, _ptr(x), _ptr(err), _ptr(child_errors)))
        return err

    def stats_ex(self, gt, sample_missing=None, multi_cap=0):
        """hpgv_stats_ex: counters + HWE, per-sample missing counts accumulated into
        `sample_missing`, and the 256-bin genotype tables of multi-allelic variants."""
        gt = _np(gt, np.uint8)
        nv, pitch = gt.shape
        c8 = np.zeros((nv, 8), np.int32)
        chi2, p = np.zeros(nv, np.float64), np.zeros(nv, np.float64)
        midx = np.zeros(max(multi_cap, 1), np.int32)
        mtab = np.zeros((max(multi_cap, 1), 256), np.int32)
        nm = C.c_int(multi_cap)
        self._chk(self.L.hpgv_stats_ex(self.h, _ptr(gt), pitch, nv, _ptr(c8), _ptr(chi2), _ptr(p),
                                       _ptr(sample_missing), _ptr(midx), _ptr(mtab), C.byref(nm)))
        k = min(nm.value, multi_cap)
        return dict(counts8=c8, hwe_chi2=chi2, hwe_p=p, n_multi=nm.value, multi_idx=midx[:k], multi_table=mtab[:k])

    def tokenize(self, text, n_samples, strict=True, max_lines=None):
        """VCF data lines (bytes) -> dict(gt [n_lines, n_samples], is_x, status, line_off, field_off, n_lines)."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        pitch = max(n_samples, 1)
        gt = np.zeros((m, pitch), np.uint8)
        is_x = np.zeros(m, np.uint8)
        line_off = np.zeros(m + 1, np.uint64)
        field_off = np.zeros((m, 10), np.uint32)
        self._chk(self.L.hpgv_tokenize(self.h, text, len(text), n_samples, 1 if strict else 0, max_lines, C.byref(nl),
                                       _ptr(line_off), _ptr(field_off), _ptr(gt), pitch, _ptr(is_x), _ptr(status)))
        res = _text_result(nl, max_lines, gt=gt[:, :n_samples], is_x=is_x, status=status, field_off=field_off)
        res["line_off"] = line_off[:len(res["status"]) + 1]                  # the end of the last line too
        return res

    def assoc_text(self, task, text, max_lines=None):
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        A1, A2, U1, U2 = (np.zeros(m, np.int32) for _ in range(4))
        odds, p = np.zeros(m, np.float64), np.zeros(m, np.float64)
        chisq = np.zeros(m, np.float64) if task == TASK_CHISQ else None
        self._chk(self.L.hpgv_assoc_text(self.h, task, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                         _ptr(A1), _ptr(A2), _ptr(U1), _ptr(U2), _ptr(odds), _ptr(chisq), _ptr(p)))
        return _text_result(nl, max_lines, status=status, A1=A1, A2=A2, U1=U1, U2=U2, odds=odds, chisq=chisq, p=p)

    def assoc_select_text(self, task, text, p_max, max_lines=None, rows_cap=None, rows_pitch=None):
        """hpgv_assoc_select_text: assoc_text's dict plus sel (per line: its number among the selected lines or -1), n_sel, and
        rows (n_sel, n_samples): the selected lines' genotype rows in VCF column order -- None when n_sel exceeds rows_cap
        (default: room for every line)."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        ns = getattr(self, "_n_samples", 0)     # (set_cohort; without one the call fails with ERR_STATE)
        if rows_cap is None:
            rows_cap = m
        if rows_pitch is None:
            rows_pitch = max(ns, 1)
        A1, A2, U1, U2 = (np.zeros(m, np.int32) for _ in range(4))
        odds, p = np.zeros(m, np.float64), np.zeros(m, np.float64)
        chisq = np.zeros(m, np.float64) if task == TASK_CHISQ else None
        sel = np.full(m, -2, np.int32)
        rows = np.full((max(rows_cap, 1), rows_pitch), 0xEE, np.uint8)
        nsel = C.c_int(0)
        self._chk(self.L.hpgv_assoc_select_text(self.h, task, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                                _ptr(A1), _ptr(A2), _ptr(U1), _ptr(U2), _ptr(odds), _ptr(chisq), _ptr(p),
                                                float(p_max), _ptr(sel), _ptr(rows), rows_pitch, rows_cap, C.byref(nsel)))
        return dict(_text_result(nl, max_lines, status=status, A1=A1, A2=A2, U1=U1, U2=U2, odds=odds, chisq=chisq, p=p, sel=sel),
                    n_sel=nsel.value, rows=rows[:nsel.value, :ns] if nsel.value <= rows_cap else None, rows_block=rows)

    def tdt_text(self, text, max_lines=None):
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        t1, t2 = np.zeros(m, np.int32), np.zeros(m, np.int32)
        odds, chisq, p = (np.zeros(m, np.float64) for _ in range(3))
        self._chk(self.L.hpgv_tdt_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                       _ptr(t1), _ptr(t2), _ptr(odds), _ptr(chisq), _ptr(p)))
        return _text_result(nl, max_lines, status=status, t1=t1, t2=t2, odds=odds, chisq=chisq, p=p)

    def tdt_perm_text(self, text, max_lines=None):
        """hpgv_tdt_perm_text: hpgv_tdt_text plus n_ge per line and batch_max per permutation."""
        text, max_lines, m, status, nl = _text_call(text, max_lines)
        t1, t2, n_ge = (np.zeros(m, np.int32) for _ in range(3))
        odds, chisq, p = (np.zeros(m, np.float64) for _ in range(3))
        np_ = getattr(self, "_n_flips", 0)
        bmax = np.zeros(max(np_, 1), np.float64)
        self._chk(self.L.hpgv_tdt_perm_text(self.h, text, len(text), max_lines, C.byref(nl), None, None, _ptr(status),
                                            _ptr(t1), _ptr(t2), _ptr(odds), _ptr(chisq), _ptr(p), _ptr(n_ge), _ptr(bmax)))
        return dict(_text_result(nl, max_lines, status=status, t1=t1, t2=t2, odds=odds, chisq=chisq, p=p, n_ge=n_ge), batch_max=bmax[:np_])

    # ---- device-resident path (raw pointers; ints or c_void_p) ---------------
    def synth(self, which, v0, n_variants, d_dst, stream=None):
        self._chk(self.L.hpgv_synth_dev(self.h, which, v0, n_variants, d_dst, stream))

    def synth_raw(self, v0, n_variants, n_samples, pitch, d_dst, stream=None):
        self._chk(self.L.hpgv_synth_raw_dev(self.h, v0, n_variants, n_samples, pitch, d_dst, stream))

    def layout(self, which, d_src, src_pitch, n_variants, d_dst, stream=None):
        self._chk(self.L.hpgv_layout_dev(self.h, which, d_src, src_pitch, n_variants, d_dst, stream))

    def assoc_scan(self, d_gt, n_variants, d_counts, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_assoc_scan_dev(self.h, d_gt, n_variants, d_is_x, d_counts, stream))

    def assoc_chisq(self, d_counts, n_variants, d_odds, d_chisq, d_p, stream=None):
        self._chk(self.L.hpgv_assoc_chisq_dev(self.h, d_counts, n_variants, d_odds, d_chisq, d_p, stream))

    def assoc_perm_dev(self, d_gt, n_variants, d_counts, d_n_ge, d_batch_max, d_perm_counts=None, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_assoc_perm_dev(self.h, d_gt, n_variants, d_is_x, d_counts, d_n_ge, d_batch_max, d_perm_counts, stream))

    def assoc_model_scan(self, d_gt, n_variants, d_counts8, stream=None):
        self._chk(self.L.hpgv_assoc_model_scan_dev(self.h, d_gt, n_variants, d_counts8, stream))

    def assoc_model_stats(self, d_counts8, n_variants, d_chisq5, d_p5, stream=None):
        self._chk(self.L.hpgv_assoc_model_stats_dev(self.h, d_counts8, n_variants, d_chisq5, d_p5, stream))

    def assoc_trend_perm_dev(self, d_gt, n_variants, d_counts8, d_n_ge, d_batch_max, d_perm_sums=None, stream=None):
        self._chk(self.L.hpgv_assoc_trend_perm_dev(self.h, d_gt, n_variants, d_counts8, d_n_ge, d_batch_max, d_perm_sums, stream))

    def assoc_cmh_dev(self, d_gt, n_variants, d_out, d_tables=None, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_assoc_cmh_dev(self.h, d_gt, n_variants, d_is_x, d_out, d_tables, stream))

    def assoc_cmh_perm_dev(self, d_gt, n_variants, d_tables, d_n_ge, d_batch_max, d_perm_chisq=None, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_assoc_cmh_perm_dev(self.h, d_gt, n_variants, d_is_x, d_tables, d_n_ge, d_batch_max, d_perm_chisq, stream))

    def assoc_logistic_dev(self, d_gt, n_variants, d_out, d_coef=None, max_iter=25, tol=1e-10, stream=None):
        self._chk(self.L.hpgv_assoc_logistic_dev(self.h, d_gt, n_variants, int(max_iter), float(tol), d_out, d_coef, stream))

    def assoc_linear_dev(self, d_gt, n_variants, d_out, d_coef=None, stream=None):
        self._chk(self.L.hpgv_assoc_linear_dev(self.h, d_gt, n_variants, d_out, d_coef, stream))

    def assoc_linear_perm_dev(self, d_gt, n_variants, d_t_obs, d_n_ge, d_batch_max, d_perm_t=None, stream=None):
        self._chk(self.L.hpgv_assoc_linear_perm_dev(self.h, d_gt, n_variants, d_t_obs, d_n_ge, d_batch_max, d_perm_t, stream))

    def ld_window_dev(self, d_gt, pitch, n_variants, window, d_r2, d_counts6=None, b_begin=0, d_chrom=None, d_pos=None, max_bp=-1,
                      d_skip=None, stream=None):
        self._chk(self.L.hpgv_ld_window_dev(self.h, d_gt, pitch, n_variants, b_begin, window, d_chrom, d_pos, int(max_bp), d_skip,
                                            d_r2, d_counts6, stream))

    def ld_edges_dev(self, d_gt, pitch, n_variants, window, min_r2, d_edges, edge_cap, d_n_edges, b_begin=0, d_chrom=None, d_pos=None,
                     max_bp=-1, d_skip=None, stream=None):
        self._chk(self.L.hpgv_ld_edges_dev(self.h, d_gt, pitch, n_variants, b_begin, window, d_chrom, d_pos, int(max_bp), d_skip,
                                           float(min_r2), d_edges, int(edge_cap), d_n_edges, stream))

    def memset_dev(self, dptr, byte_value, nbytes, stream=None):
        self._chk(self.L.hpgv_memset_dev(self.h, dptr, byte_value, nbytes, stream))

    def ibs_pairs_dev(self, d_gt, pitch, n_variants, n_cols, d_counts, d_skip=None, stream=None):
        self._chk(self.L.hpgv_ibs_pairs_dev(self.h, d_gt, pitch, n_variants, n_cols, d_skip, d_counts, stream))

    def ibs_class_counts_dev(self, d_gt, pitch, n_variants, n_cols, d_class4, d_skip=None, stream=None):
        self._chk(self.L.hpgv_ibs_class_counts_dev(self.h, d_gt, pitch, n_variants, n_cols, d_skip, d_class4, stream))

    def grm_table_dev(self, d_class4, n_variants, frac_bits, min_maf, d_skip, d_tab, d_n_used=None, stream=None):
        self._chk(self.L.hpgv_grm_table_dev(self.h, d_class4, n_variants, int(frac_bits), float(min_maf), d_skip, d_tab, d_n_used, stream))

    def grm_pairs_dev(self, d_gt, pitch, n_variants, n_cols, d_tab, d_acc, d_skip=None, stream=None):
        self._chk(self.L.hpgv_grm_pairs_dev(self.h, d_gt, pitch, n_variants, n_cols, d_skip, d_tab, d_acc, stream))

    def score_table_dev(self, d_class4, n_variants, d_w, d_flags, frac_bits, impute, d_skip, d_tab, tab_pitch, d_const, stream=None, n_scores=None):
        s = _np(frac_bits, np.int32).reshape(-1)
        self._chk(self.L.hpgv_score_table_dev(self.h, d_class4, n_variants, d_w, d_flags, len(s) if n_scores is None else int(n_scores), _ptr(s),
                                              1 if impute else 0, d_skip, d_tab, tab_pitch, d_const, stream))

    def score_cols_dev(self, d_gt, pitch, n_variants, n_cols, d_tab, tab_pitch, n_scores, d_acc, acc_pitch, d_skip=None, stream=None):
        self._chk(self.L.hpgv_score_cols_dev(self.h, d_gt, pitch, n_variants, n_cols, d_skip, d_tab, tab_pitch, int(n_scores), d_acc, acc_pitch, stream))

    def grm_matrix_dev(self, d_acc, n_cols, frac_bits, d_A, lda, d_n_empty, stream=None):
        self._chk(self.L.hpgv_grm_matrix_dev(self.h, d_acc, n_cols, int(frac_bits), d_A, lda, d_n_empty, stream))

    def pca_apply_dev(self, d_A, n, lda, d_Q, L, d_Y, stream=None):
        self._chk(self.L.hpgv_pca_apply_dev(self.h, d_A, n, lda, d_Q, L, d_Y, stream))

    def pca_dev(self, d_A, n, lda, k, tol=1e-8, max_iter=1000, seed=1):
        """hpgv_pca_dev: dict of eigval (k,), vec (n, k), resid (k,), n_iter, converged"""
        kk = max(int(k), 1)
        eigval, vec, resid = np.zeros(kk), np.zeros((max(n, 1), kk)), np.zeros(kk)
        it, conv = C.c_int(0), C.c_int(0)
        self._chk(self.L.hpgv_pca_dev(self.h, d_A, n, lda, int(k), float(tol), int(max_iter), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(eigval), _ptr(vec), _ptr(resid),
                                      C.byref(it), C.byref(conv)))
        return dict(eigval=eigval, vec=vec[:n], resid=resid, n_iter=it.value, converged=conv.value)

    def ibs_select_dev(self, d_counts, n_cols, E, min_pi_hat, d_pairs, cap, d_n, stream=None):
        e = _np(E, np.float64)
        self._chk(self.L.hpgv_ibs_select_dev(self.h, d_counts, n_cols, _ptr(e), float(min_pi_hat), d_pairs, int(cap), d_n, stream))

    def rows_gather_scratch_bytes(self, n_rows):
        return self.L.hpgv_rows_gather_scratch_bytes(n_rows)

    def rows_gather_dev(self, d_src, src_pitch, row_bytes, n_rows, d_keep, d_dst, dst_pitch, d_index, d_n_kept, d_scratch, stream=None):
        self._chk(self.L.hpgv_rows_gather_dev(self.h, d_src, src_pitch, row_bytes, n_rows, d_keep, d_dst, dst_pitch, d_index, d_n_kept,
                                              d_scratch, stream))

    def assoc_fisher(self, d_counts, n_variants, d_odds, d_p, stream=None):
        self._chk(self.L.hpgv_assoc_fisher_dev(self.h, d_counts, n_variants, d_odds, d_p, stream))

    def inflate_blocks(self, d_comp, d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_text, d_status, stream=None):
        self._chk(self.L.hpgv_inflate_blocks_dev(self.h, d_comp, d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_text, d_status, stream))

    def bgzf_verify_tiles(self, d_comp, d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_text, d_status, d_tiles, n_tiles, stream=None):
        self._chk(self.L.hpgv_bgzf_verify_tiles_dev(self.h, d_comp, d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_text, d_status, d_tiles, n_tiles, stream))

    def bgzf_verify(self, d_comp, d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_text, d_status, stream=None):
        self._chk(self.L.hpgv_bgzf_verify_dev(self.h, d_comp, d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_text, d_status, stream))

    def bgzf_scan(self, d_comp, lo, hi, text_base, max_rows, d_in_off, d_in_len, d_out_off, d_out_len, stream=None):
        """Rows of the decoder's tables for the chain of bgzip blocks from byte lo that end by hi -> (rows, chain end, text end, headers seen)."""
        need = self.L.hpgv_bgzf_scan_scratch_bytes(hi - lo, max_rows)
        scratch = self.alloc(need)
        res = np.zeros(4, np.uint64)
        try:
            self._chk(self.L.hpgv_bgzf_scan_dev(self.h, d_comp, lo, hi, text_base, max_rows, d_in_off, d_in_len, d_out_off, d_out_len,
                                                scratch, need, _ptr(res), stream))
        finally:
            self.free(scratch)
        return tuple(int(x) for x in res)

    def dev_reserve(self, max_bytes):
        p = C.c_void_p()
        self._chk(self.L.hpgv_dev_reserve(self.h, max_bytes, C.byref(p)))
        return p

    def dev_commit(self, p, nbytes):
        self._chk(self.L.hpgv_dev_commit(self.h, p, nbytes))

    def dev_release(self, p):
        self._chk(self.L.hpgv_dev_release(self.h, p))

    def tdt_scan(self, d_gt, n_variants, d_tu, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_tdt_scan_dev(self.h, d_gt, n_variants, d_is_x, d_tu, stream))

    def tdt_stats(self, d_tu, n_variants, d_odds, d_chisq, d_p, stream=None):
        self._chk(self.L.hpgv_tdt_stats_dev(self.h, d_tu, n_variants, d_odds, d_chisq, d_p, stream))

    def tdt_perm_dev(self, d_gt, n_variants, d_tu, d_n_ge, d_batch_max, d_perm_tu=None, d_is_x=None, stream=None):
        self._chk(self.L.hpgv_tdt_perm_dev(self.h, d_gt, n_variants, d_is_x, d_tu, d_n_ge, d_batch_max, d_perm_tu, stream))

    def stats_scan(self, d_gt, n_variants, d_counts8, stream=None):
        self._chk(self.L.hpgv_stats_scan_dev(self.h, d_gt, n_variants, d_counts8, stream))

    def stats_hwe(self, d_counts8, n_variants, d_chi2, d_p, stream=None):
        self._chk(self.L.hpgv_stats_hwe_dev(self.h, d_counts8, n_variants, d_chi2, d_p, stream))

    def sample_missing(self, d_gt, n_variants, d_missing, stream=None):
        self._chk(self.L.hpgv_sample_missing_dev(self.h, d_gt, n_variants, d_missing, stream))

    def genotype_table(self, d_raw, src_pitch, n_samples, d_idx, n_idx, d_table, stream=None):
        self._chk(self.L.hpgv_genotype_table_dev(self.h, d_raw, src_pitch, n_samples, d_idx, n_idx, d_table, stream))

    def stats_filter(self, d_counts8, n_variants, d_keep, min_maf=-1.0, max_maf=-1.0, max_missing=-1.0, stream=None):
        self._chk(self.L.hpgv_stats_filter_dev(self.h, d_counts8, n_variants, min_maf, max_maf, max_missing, d_keep, stream))

    def inheritance_scan(self, d_gt, n_variants, d_counts8, stream=None):
        self._chk(self.L.hpgv_inheritance_scan_dev(self.h, d_gt, n_variants, d_counts8, stream))

    def last_kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        self._chk(self.L.hpgv_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- group context: the variant-sharded resident scan (hpgv_group_*) ---------------------------------
    def group_size(self):
        return self.L.hpgv_group_size(self.h)

    def member(self, i):
        """Engine view of member i of a group context (its device memory, generator, *_dev calls); owned by the group."""
        h = self.L.hpgv_group_member(self.h, i)
        if not h:
            raise HpgvError("no member %d" % i)
        m = Engine.__new__(Engine)
        m.L, m.h, m.device, m._bufs, m._host_bufs, m._view = self.L, C.c_void_p(h), self.L.hpgv_member_device(self.h, i), [], [], True
        m._views = []
        m._parent = self                # the view keeps its group alive; the group's close() closes its views first
        self._views.append(m)
        return m

    def group_comm_init(self):
        self._chk(self.L.hpgv_group_comm_init(self.h))
        return self.L.hpgv_group_comm_ranks(self.h)

    def group_shard(self, n_variants, member):
        lo, hi = C.c_int64(), C.c_int64()
        self._chk(self.L.hpgv_group_shard(self.h, n_variants, member, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    @staticmethod
    def _ptr_array(ptrs):
        if ptrs is None:
            return None
        return (C.c_void_p * len(ptrs))(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])

    def group_assoc(self, task, d_gt, n_variants, d_counts, d_odds, d_chisq, d_p, d_is_x=None):
        self._chk(self.L.hpgv_group_assoc(self.h, task, self._ptr_array(d_gt), self._ptr_array(d_is_x), n_variants,
                                          d_counts, d_odds, d_chisq, d_p))

    def group_tdt(self, d_gt, n_variants, d_tu, d_odds, d_chisq, d_p, d_is_x=None):
        self._chk(self.L.hpgv_group_tdt(self.h, self._ptr_array(d_gt), self._ptr_array(d_is_x), n_variants, d_tu, d_odds, d_chisq, d_p))

    def group_stats(self, d_gt, n_variants, d_counts8, d_chi2, d_p, d_sample_missing=None):
        self._chk(self.L.hpgv_group_stats(self.h, self._ptr_array(d_gt), n_variants, d_counts8, d_chi2, d_p, d_sample_missing))

    def group_epi_share(self, order, member):
        lo, hi = C.c_int(), C.c_int()
        self._chk(self.L.hpgv_group_epi_share(self.h, order, member, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def group_epi_rank(self, order, subset, max_ranking_size):
        k, n = self._epi[3], max_ranking_size
        combs = np.zeros((k, n, order), np.int32)
        acc, mask, cnt = np.zeros((k, n), np.float64), np.zeros((k, n, 8), np.uint32), np.zeros(k, np.int32)
        ms = C.c_float(0)
        self._chk(self.L.hpgv_group_epi_rank(self.h, order, subset, n, _ptr(combs), _ptr(acc), _ptr(mask), _ptr(cnt), C.byref(ms)))
        return dict(combs=combs, accuracy=acc, risky=mask, n=cnt, scan_ms=ms.value)

    def group_sync(self):
        self._chk(self.L.hpgv_group_sync(self.h))

    def mfma_f64_probe(self, steps=4096, iters=5):
        """hpgv_mfma_f64_probe: (kernel ms, flop per launch) of the f64 matrix cores with no memory traffic"""
        ms, flop = C.c_float(), C.c_double()
        self._chk(self.L.hpgv_mfma_f64_probe(self.h, steps, iters, C.byref(ms), C.byref(flop)))
        return ms.value, flop.value

    def read_probe(self, d_buf, nbytes, iters=5):
        ms = C.c_float()
        self._chk(self.L.hpgv_read_probe(self.h, d_buf, nbytes, iters, C.byref(ms)))
        return ms.value
