/*
 * hpgv.h -- C ABI of the MI355X-native per-variant statistics engine.
 *
 * This is the drop-in boundary for opencb/hpg-variant's per-batch hot path.
 * Each entry point names the reference interface it stands behind (paths are
 * relative to the reference tree):
 *
 *   hpgv_assoc*      <- assoc_test()            src/gwas/assoc/assoc.h:137-138, assoc.c:23-84
 *                       assoc_count_individual  src/gwas/assoc/assoc.c:87-134
 *                       assoc_basic_test/result src/gwas/assoc/assoc_basic_test.c:23-64
 *                       assoc_fisher_test       src/gwas/assoc/assoc_fisher_test.c:24-26
 *   hpgv_set_logfact <- init_logarithm_array()  call site src/gwas/assoc/assoc_runner.c:164-166
 *   hpgv_tdt*        <- tdt_test()              src/gwas/tdt/tdt.h:119, tdt.c:23-276
 *                       tdt_result_new          src/gwas/tdt/tdt.c:279-295
 *   hpgv_stats*      <- get_variants_stats()    call site src/vcf-tools/stats/stats_runner.c:194-195
 *   hpgv_set_cohort  <- sort_individuals() + individual->condition
 *                                               src/gwas/assoc/assoc_runner.c:138-140, assoc.c:95,101
 *   hpgv_set_families<- ped_flatten_families() + family->founders/members walk
 *                                               src/gwas/tdt/tdt_runner.c:87, tdt.c:56-95,135-148
 *
 * Plain C: opaque context, plain pointers and sizes, int status codes, caller
 * allocated outputs.  No function aborts; hpgv_last_error() gives the text.
 * The library has NO CPU fallback: without a usable HIP device hpgv_create()
 * fails with HPGV_ERR_NO_DEVICE.
 *
 * Genotype code (one byte per call, "HPGV8"):
 *      byte = (allele1 << 4) | allele2      allele index 0..14 (larger ones are stored as 14; two DIFFERENT alleles
 *                                           above 13 as 13/14, so that "15/16" stays heterozygous: tdt.c:113,185-187),
 *      nibble 0xF = missing allele, 0xFF = missing / unusable genotype.
 *   Biallelic data uses 0x00 0x01 0x10 0x11 0xFF.  The ORDER of the alleles is
 *   kept because tdt.c:119,176-213 tests them in order.
 */
#ifndef HPGV_H
#define HPGV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPGV_GT_MISSING 0xFF

/* status codes */
enum {
    HPGV_OK = 0,
    HPGV_ERR_INVALID = 1,      /* bad argument */
    HPGV_ERR_NO_DEVICE = 2,    /* no usable HIP device */
    HPGV_ERR_HIP = 3,          /* a HIP runtime call failed */
    HPGV_ERR_NOMEM = 4,
    HPGV_ERR_STATE = 5,        /* e.g. scan before the cohort was set */
    HPGV_ERR_UNSUPPORTED = 6   /* shape outside the engine's limits */
};

/* enum ASSOC_task of assoc.h:55 */
enum { HPGV_TASK_NONE = 0, HPGV_TASK_CHISQ = 1, HPGV_TASK_FISHER = 2 };
/* individual->condition / ->sex by meaning (hpg-libs enums are not in the tree) */
enum { HPGV_COND_UNAFFECTED = 0, HPGV_COND_AFFECTED = 1, HPGV_COND_OTHER = 2 };
enum { HPGV_SEX_MALE = 0, HPGV_SEX_FEMALE = 1, HPGV_SEX_UNKNOWN = 2 };

typedef struct hpgv_ctx hpgv_ctx;

/* ---- lifetime ------------------------------------------------------------ */
const char *hpgv_version(void);
int  hpgv_device_count(void);                       /* <0 on HIP failure */
int  hpgv_create(int device_id, hpgv_ctx **out);
/* Several devices behind ONE context ("the context owns the devices"; the reference's runner deals its
 * batches to num_threads workers, assoc_runner.c:106-207 -- here they land on n_devices GPUs).  A group context takes
 * every call an ordinary one takes:
 *   - cohort / option calls (hpgv_set_*) are applied to every member device;
 *   - the synchronous per-batch entry points (hpgv_assoc, hpgv_tdt, hpgv_stats*, hpgv_mendel, hpgv_epi_dataset,
 *     hpgv_tokenize, hpgv_*_text) run on the member with the fewest calls in flight, so concurrent worker threads spread
 *     over the devices; variants are independent (assoc.c:38-82), so no exchange between devices is needed, and the
 *     per-sample counters of hpgv_stats_ex / hpgv_stats_text are accumulated into the caller's host arrays by every call;
 *   - device memory, streams, the device-resident entry points (hpgv_*_dev), hpgv_text_alias and the epistasis calls
 *     refer to member 0; hpgv_group_member gives the context of another member for device-resident work there.
 * The same device id may be listed more than once (two contexts on one device: what the tests do on a one-GPU box).
 * hpgv_destroy of the group destroys its members; a member must not be destroyed on its own. */
int  hpgv_create_multi(const int *device_ids, int n_devices, hpgv_ctx **out);
int  hpgv_group_size(const hpgv_ctx *ctx);                 /* 1 for an ordinary context */
hpgv_ctx *hpgv_group_member(hpgv_ctx *ctx, int i);         /* NULL when out of range */
int  hpgv_member_device(const hpgv_ctx *ctx, int i);       /* device id of member i, -1 when out of range */
void hpgv_destroy(hpgv_ctx *ctx);
/* text of the last failure on this ctx (ctx == NULL: last hpgv_create failure
 * of the calling thread) */
const char *hpgv_last_error(const hpgv_ctx *ctx);
/* Options of a context (key, value; before the cohort is set where noted):
 *   "row_align"   bytes, power of two >= 16 (default 16; before the cohort)      "row_pad"  extra bytes per row, multiple of 16
 *   "variants_per_wave" (default 2), "blocks_per_cu" (1..8), "scan_lds"          launch shape of the resident scans
 *   "profile" 0/1                HIP events around the scan / statistics kernels (hpgv_last_kernel_ms)
 *   "fisher_cut_exp" 12..300     a Fisher tail stops below 10^-this of its largest term (default 22: below one ulp of the sum)
 *   "batch_fused" 0/1, "batch_copy" 0/1   per-batch host entry points: one fused kernel reading page-locked rows in place
 *                                (default) / the kernel chain / copy the rows first
 *   "epi_complete" 0/1, "epi_triples_1pass" 0/1     epistasis scans: the shortcuts for data without missing calls / <= 10 folds
 *   "epi_pairs_mfma", "epi_triples_mfma" 0/1 (default 1)   epistasis pair / triple ranking: cell counts on the matrix cores (0: the vector-ALU scans;
 *                                    whatever the option, the vector ALU when a class holds 65 536 samples or more or the
 *                                    samples with their padding need more than 128 staging chunks or the genotype planes'
 *                                    second copy finds no room: hpgv_epi_last_rank_info says which ran)
 *   "epi_wide" 0/1/2 (default 0)  epistasis past the packed kernels' limits (16 folds; 16-bit counts: fewer than 65 536 samples per (fold, class)
 *                                    group, at most 65 535 per class for triples and listed combinations).  0: those limits hold and are refused.
 *                                    1: up to 64 folds and groups / classes of any size -- such shapes run on the wide listed-combination
 *                                    kernel (k_epi_combs_wide: 32-bit counts), see "Wide limits" at the epistasis entry points; every shape
 *                                    the packed kernels take keeps them.  2: the wide kernel for EVERY listed-combination launch (tests,
 *                                    measurement).  On a group context the option goes to every member.  hpgv_run_epistasis[_order] of
 *                                    the host library set 1 for their run.
 *   "group_self_exchange" 0/1    (group contexts; tests) member 0 hands its results over through the communicator too
 *   "group_fake_ranks" n         (group contexts; tests) 0 (default): communicator ranks by distinct device.  n >= 1: the first n
 *                                members share rank 0 and every later member is a rank of its own, whatever its device, so the
 *                                device list handed to ncclCommInitAll may repeat a device -- which RCCL refuses and only a
 *                                stand-in communicator (HPGV_RCCL_LIB) accepts.  Before the communicator exists
 *                                (hpgv_group_comm_init or the first group call); afterwards HPGV_ERR_STATE
 *   "part_aligned_loads" 0/1     hpgv_lines_partition_dev: the source of a granule by two aligned loads and v_alignbyte
 *                                (ablation build) instead of one unaligned dwordx4 load (shipped: 0)
 *   "pca_apply_vector" 0/1       hpgv_pca_apply_dev: the lane-per-row v_fma_f64 form (ablation build) instead of the f64
 *                                matrix-core form (shipped: 0)
 * Every kernel ships in ONE form.  The forms that lost their A/B comparisons (profiles/experiments_that_did_not_pay.md) are
 * compiled only into an ablation build (-DHPGV_ABLATION: tools/build_ablation.py, used by tools/ only); there the keys
 * "pipeline", "persistent", "scan_unroll", "pipe_waves", "nontemporal", "fisher_width", "inflate_wave", "tokenizer_tiles",
 * "pca_apply_vector" select them, and in the shipped library any value but the shipped one is refused with HPGV_ERR_UNSUPPORTED.
 *
 * Environment.  The library reads the environment in exactly two places: hpgv_create (the table below, once per context,
 * into the context) and hpgv_group_comm_init (HPGV_RCCL_LIB).  No entry point that launches work reads it.
 *   HPGV_BATCH_FUSED=0        as option "batch_fused" 0: the per-batch calls as a chain of kernels       (default 1)
 *   HPGV_BATCH_COPY=1         as option "batch_copy" 1                                                    (default 0)
 *   HPGV_STATS_ALL2=0         every stats batch through the row-staging kernel k_stats_all -- the fall-back of the shapes
 *                             k_stats_all2 does not take (unaligned rows, very wide cohorts, > 3 masked groups)  (default 1)
 *   HPGV_ASSOC_ROWS=0         text batches counted one workgroup per row (k_batch) -- the fall-back of cohorts wider than
 *                             k_assoc_rows takes                                                          (default 1)
 *   HPGV_PINNED_NONCOHERENT=1 hpgv_host_alloc asks for non-coherent page-locked memory                   (default 0)
 *   HPGV_VMM_TRACE=1          hpgv_dev_commit narrates its mappings on stderr                             (default 0)
 *   HPGV_DECODE_TILES=0       windows of text the bgzip decoder left with its tile records (hpgv_text_alias_tiles) are
 *                             tokenized with the counting sweep all the same (A/B of that short cut)     (default 1)
 *   HPGV_RCCL_LIB=<path>      librccl to load first (then the librccl beside the HIP runtime this library is bound to,
 *                             then librccl.so.1, librccl.so, /opt/rocm/lib/...)
 * (libhpgv_host.so has a table of its own: include/hpgv_host.h "Environment".) */
int  hpgv_set_option(hpgv_ctx *ctx, const char *key, long value);

/* ---- cohort description (replicated per device; tiny) --------------------- */
/* condition[j] for VCF column j (HPGV_COND_*).  Builds the assoc layout:
 * [affected columns | pad to 16 B | unaffected columns | pad], others dropped. */
int  hpgv_set_cohort(hpgv_ctx *ctx, const uint8_t *condition, int n_samples);
int  hpgv_assoc_layout(const hpgv_ctx *ctx, int *n_affected, int *n_unaffected, size_t *pitch);

/* Families in CSR form, already filtered the way tdt.c does: family f has VCF
 * columns father_col[f] / mother_col[f] (<0: founder missing or not in the VCF,
 * family skipped, tdt.c:77-95) and its counted children
 * child_off[f]..child_off[f+1]-1 = members with both parents set, AFFECTED and
 * present in the VCF (tdt.c:139-148), in family->members iteration order. */
int  hpgv_set_families(hpgv_ctx *ctx, int n_samples, int n_families,
                       const int32_t *father_col, const int32_t *mother_col,
                       const int32_t *child_off, const int32_t *child_col,
                       const uint8_t *child_sex);
int  hpgv_tdt_layout(const hpgv_ctx *ctx, int *n_trios_fast, int *n_families_slow, size_t *pitch);

/* table[i] = ln(i!) for i < n, as init_logarithm_array(num_samples*10) builds it.
 * Must cover 2*n_samples+1 entries for the Fisher pass. */
int  hpgv_set_logfact(hpgv_ctx *ctx, const double *table, size_t n);

/* stats layout: all n_samples columns in VCF order, pad to 16 B */
int  hpgv_set_stats_cohort(hpgv_ctx *ctx, int n_samples);
int  hpgv_stats_layout(const hpgv_ctx *ctx, size_t *pitch);

/* per-phenotype statistics (stats_runner.c:47-98,300-303,319-323 write one report per phenotype
 * group): group_of_sample[j] in [0, n_groups) or < 0 for "in no group".  Builds the layout
 * HPGV_LAYOUT_STATS_GROUPS = [group 0 columns | pad16 | group 1 columns | pad16 | ...]. */
int  hpgv_set_stats_groups(hpgv_ctx *ctx, const int32_t *group_of_sample, int n_samples, int n_groups);
int  hpgv_stats_groups_layout(const hpgv_ctx *ctx, size_t *pitch, int *group_sizes /* n_groups ints, may be NULL */);

/* Mendelian errors (hpg-libs check_mendel: the --mendel filter of shared_options.c:45,101-105 and the
 * per-sample counter of get_sample_stats): every child with both parents among the VCF columns is one
 * trio, whatever its phenotype.  Layout HPGV_LAYOUT_MENDEL = [father | mother | child] class planes. */
int  hpgv_set_pedigree(hpgv_ctx *ctx, int n_samples, int n_trios, const int32_t *father_col,
                       const int32_t *mother_col, const int32_t *child_col, const uint8_t *child_sex);
int  hpgv_mendel_layout(const hpgv_ctx *ctx, size_t *pitch);

/* ---- device memory + streams (thin; callers may also pass memory owned by
 *      another runtime, e.g. a torch tensor's data_ptr) ---------------------- */
int  hpgv_dev_alloc(hpgv_ctx *ctx, size_t bytes, void **dptr);
int  hpgv_dev_free(hpgv_ctx *ctx, void *dptr);
int  hpgv_memset_dev(hpgv_ctx *ctx, void *dptr, int byte_value, size_t bytes, void *stream);   /* stream NULL: done when it returns */
/* device memory that grows in place: reserve an address range of max_bytes (costs no memory), make its first `bytes` bytes
 * usable with hpgv_dev_commit (what is backed stays backed; pieces of 64 MB), give everything back with hpgv_dev_release.
 * For a text whose size is known only when its last block has been seen.  HPGV_ERR_UNSUPPORTED: no virtual memory management.
 * hpgv_dev_commit fails with HPGV_ERR_NOMEM when the memory is not there; the pieces it mapped before failing stay mapped
 * (hpgv_dev_committed).  Sizes are rounded to the device's allocation granularity (hipMemGetAllocationGranularity). */
int  hpgv_dev_reserve(hpgv_ctx *ctx, size_t max_bytes, void **dptr);
int  hpgv_dev_commit(hpgv_ctx *ctx, void *dptr, size_t bytes);
int  hpgv_dev_committed(hpgv_ctx *ctx, void *dptr, size_t *bytes);   /* how far the range is backed (a failed commit may have grown it) */
int  hpgv_dev_release(hpgv_ctx *ctx, void *dptr);
int  hpgv_memcpy_h2d(hpgv_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);
int  hpgv_memcpy_d2h(hpgv_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);
int  hpgv_memcpy_h2d_async(hpgv_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream);   /* queued only; src page-locked and left alone until hpgv_stream_sync */
int  hpgv_stream_sync(hpgv_ctx *ctx, void *stream);   /* stream NULL = default stream */
/* page-locked host memory: buffers handed to the host entry points copy to the device at full
 * PCIe rate when they come from here (pageable memory is staged by the driver, 2-4x slower) */
/* NUMA node of the device (-1: unknown).  No reference counterpart: the file runners put their staging threads and
 * page-locked buffers there (a copy out of the page cache into buffers on the other socket ran at half the rate) */
int  hpgv_device_numa_node(hpgv_ctx *ctx, int *node);
/* a non-blocking stream of the caller's own, e.g. for copies that overlap the engine's work */
int  hpgv_stream_create(hpgv_ctx *ctx, void **stream);
int  hpgv_stream_create_low(hpgv_ctx *ctx, void **stream);      /* lowest priority: its kernels give way to the other streams' */
int  hpgv_stream_destroy(hpgv_ctx *ctx, void *stream);
int  hpgv_host_alloc(hpgv_ctx *ctx, size_t bytes, void **hptr);
int  hpgv_host_free(hpgv_ctx *ctx, void *hptr);

/* ---- layout kernels: VCF-order code matrix (device) -> engine layout ------ */
/* which: 0 assoc, 1 tdt, 2 stats, 3 stats by phenotype group, 4 Mendelian-error trios,
 * 5 epistasis dataset (assoc column order, vcf2epi codes 0/1/2/255; pads 255).  d_src rows are src_pitch bytes apart and hold
 * n_samples codes in VCF column order; d_dst rows use the layout's pitch. */
enum { HPGV_LAYOUT_ASSOC = 0, HPGV_LAYOUT_TDT = 1, HPGV_LAYOUT_STATS = 2, HPGV_LAYOUT_STATS_GROUPS = 3,
       HPGV_LAYOUT_MENDEL = 4, HPGV_LAYOUT_EPI = 5 };
int  hpgv_layout_dev(hpgv_ctx *ctx, int which, const uint8_t *d_src, size_t src_pitch,
                     int n_variants, uint8_t *d_dst, void *stream);

/* ---- synthetic cohort generator, written directly in the
 *      engine layout `which`; variant ids v0..v0+n_variants-1 ------------------ */
int  hpgv_synth_dev(hpgv_ctx *ctx, int which, uint64_t v0, int n_variants,
                    uint8_t *d_dst, void *stream);
/* same genotypes in plain VCF column order (for staging tests) */
int  hpgv_synth_raw_dev(hpgv_ctx *ctx, uint64_t v0, int n_variants, int n_samples,
                        size_t pitch, uint8_t *d_dst, void *stream);

/* ---- the hot path on device-resident data (asynchronous on `stream`) ------ */
/* scan: d_gt in assoc layout -> d_counts[v] = {A1, A2, U1, U2} (int32 x4).
 * d_is_x: per-variant flag "chromosome is exactly X" (assoc.c:94) or NULL. */
int  hpgv_assoc_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants,
                         const uint8_t *d_is_x, int32_t *d_counts, void *stream);
/* statistics from the counts; SoA outputs of n_variants doubles each */
int  hpgv_assoc_chisq_dev(hpgv_ctx *ctx, const int32_t *d_counts, int n_variants,
                          double *d_odds, double *d_chisq, double *d_p, void *stream);
int  hpgv_assoc_fisher_dev(hpgv_ctx *ctx, const int32_t *d_counts, int n_variants,
                           double *d_odds, double *d_p, void *stream);

/* ---- label permutation of the chi-square association test: max(T) empirical p-values (PLINK's --mperm; no reference
 *      counterpart).  For a 0/1 labelling p of the COHORT columns (those whose condition in hpgv_set_cohort is AFFECTED or
 *      UNAFFECTED; HPGV_COND_OTHER columns take no part under any labelling) the permuted counts are
 *          A1_p(v) = sum_j c1(v, j) y_p(j),   A2_p(v) = sum_j c2(v, j) y_p(j)
 *      with the per-sample contributions (c1, c2) of column j's HPGV8 byte
 *          autosome: c1 = nibbles equal to 0, c2 = nibbles that are neither 0 nor 0xF       (0xFF: 0, 0)
 *          chr X   : c1 = 1 for byte 0x00, c2 = 1 for a byte whose nibbles are both neither 0 nor 0xF
 *      (summed over the affected columns they are hpgv_assoc_scan_dev's {A1, A2}, over the unaffected ones {U1, U2}): an i8
 *      matrix product with exact i32 sums on the matrix cores (csrc/hpgv_assoc_perm_kernels.h).  The permuted table is
 *      a = A1_p, c = A2_p, b = R1 - A1_p, d = R2 - A2_p with R1 = A1 + U1, R2 = A2 + U2 of the observed counts;
 *      T_p(v) is the chi-square of that table by the device function hpgv_assoc_chisq_dev uses, T_obs(v) the same on the
 *      observed counts.  A NaN T_p(v) (an empty margin) is never >= anything and never enters a maximum.  Outputs per call:
 *          n_ge[v]      = #{p : T_p(v) >= T_obs(v)}  (int32; 0 when T_obs(v) is NaN)
 *          batch_max[p] = max over the call's variants of T_p(v)  (0.0 when every value is NaN or the call has no variants)
 *      Calls are stateless: a scan in several batches sums nothing and merges batch_max by element-wise maximum (0 is the
 *      identity: chi-square is never negative); hpgv_perm_pvalues turns the merged maxima into p-values. */
/* labels[p * n_samples + j] in {0, 1} for VCF column j (ignored for HPGV_COND_OTHER columns), one row per permutation; a row
 * need not keep the number of affected samples.  After hpgv_set_cohort (else HPGV_ERR_STATE); a group context gives every
 * member the labels, as it does the cohort.  n_perms == 0 drops the labels; so does a new hpgv_set_cohort.  A value above 1
 * in a cohort column: HPGV_ERR_INVALID.  Limits: more than 1 048 576 permutations per call is HPGV_ERR_UNSUPPORTED; the label
 * matrix takes (n_perms rounded up to 16) x the assoc layout's pitch bytes of device memory and HPGV_ERR_NOMEM is returned
 * when they are not there.  Not to be called while permutation calls of the context are in flight. */
int  hpgv_set_perm_labels(hpgv_ctx *ctx, const uint8_t *labels, int n_perms);
/* d_gt in assoc layout, d_counts what hpgv_assoc_scan_dev wrote for it -> d_n_ge (n_variants int32), d_batch_max (n_perms
 * doubles), both overwritten.  d_perm_counts (may be NULL; for tests and for callers who want another statistic):
 * {A1_p, A2_p} as int32[(v * n_perms + p) * 2 + k].  d_gt and d_counts 16-byte aligned, d_batch_max and d_perm_counts
 * 8-byte aligned.  Asynchronous on `stream`.  HPGV_ERR_STATE without labels.  The launch reads the genotype matrix
 * ceil(n_perms / 128) times. */
int  hpgv_assoc_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_counts,
                         int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_counts /* may be NULL */, void *stream);

/* ---- model tests: the genotypic tests of a case/control scan (PLINK's --model; no reference counterpart).  The allelic
 *      chi-square counts every diploid sample twice and so assumes Hardy-Weinberg equilibrium; these work on genotypes.
 *
 *      Genotype class of an HPGV8 byte, in any layout:
 *          missing      either nibble is 0xF (this covers 0xFF and the layout's pad bytes)
 *          0 (hom-ref)  byte 0x00
 *          1 (het)      exactly one nibble is 0 and the other is in 1..14
 *          2 (hom-alt)  both nibbles are in 1..14 ("1/2" counts as hom-alt, as assoc.c:112 counts it as two alternate alleles)
 *      Dosage equals the class index.  Chromosome X gets no special rule, because these are genotype tests: d_is_x is not a
 *      parameter of any call below.
 *
 *      Counts per variant, int32 x 8:  {r0, r1, r2, s0, s1, s2, miss_aff, miss_unaff}
 *      r counts the affected cohort columns and s the unaffected ones; miss_* counts the group's real columns whose genotype
 *      is missing (pads are never counted).  On a row in the assoc layout 2 r0 + r1 == A1, r1 + 2 r2 == A2, 2 s0 + s1 == U1
 *      and s1 + 2 s2 == U2 of hpgv_assoc_scan_dev with d_is_x == NULL.
 *
 *      Statistics.  R = sum r, S = sum s, N = R + S, n_k = r_k + s_k.  Five tests in a fixed order (HPGV_MODEL_*);
 *      chisq5[v][t] and p5[v][t] are doubles, everything is f64 without contraction.  Nothing is rejected for small cells: a
 *      zero margin gives 0 / 0 = NaN with p = NaN, as the allelic chi-square already does.
 *          GENO     Pearson chi-square of the 2 x 3 table, each expected value rowtot * coltot / N.
 *                   df 2: p = exp(-chi2 / 2), NaN in gives NaN out, chi2 <= 0 gives 1
 *          TREND    Cochran-Armitage, weights 0, 1, 2.  With W1 = n1 + 2 n2, W2 = n1 + 4 n2, D = r1 + 2 r2:
 *                   chi2 = N (N D - R W1)^2 / (R (N - R) (N W2 - W1^2)).                      df 1, p as hpgv_assoc_chisq_dev's
 *          ALLELIC  the chi-square of hpgv_assoc_chisq_dev on (2 r0 + r1, r1 + 2 r2, 2 s0 + s1, s1 + 2 s2): the same device
 *                   function and argument order, so it equals hpgv_assoc's chisq bit for bit on non-X rows.   df 1
 *          DOM      the same function on (r1 + r2, r0, s1 + s2, s0).                                          df 1
 *          REC      the same function on (r2, r0 + r1, s2, s0 + s1).                                          df 1
 *
 *      Trend permutation.  Under a labelling y_p (the rows of hpgv_set_perm_labels: same state, same limits, same rules for
 *      HPGV_COND_OTHER columns)
 *          R_p = sum_j valid(v, j) y_p(j),   D_p = sum_j dosage(v, j) y_p(j)
 *      an i8 product on the matrix cores as the label permutation's; T_p = the TREND statistic with (R, D) replaced by
 *      (R_p, D_p) -- N, W1 and W2 do not depend on the labels -- and T_obs the same function on the observed (R, D).  Outputs,
 *      NaN rules and merge rule are those of hpgv_assoc_perm_dev: n_ge[v] overwritten, batch_max[p] 0.0 when nothing enters,
 *      batches merge by element-wise maximum, then hpgv_perm_pvalues. */
enum { HPGV_MODEL_GENO = 0, HPGV_MODEL_TREND = 1, HPGV_MODEL_ALLELIC = 2, HPGV_MODEL_DOM = 3, HPGV_MODEL_REC = 4 };
/* d_gt in assoc layout -> d_counts8[v] (int32 x 8), both 16-byte aligned.  A cohort whose rows have more than 262 080 16-byte
 * chunks is HPGV_ERR_UNSUPPORTED (the scan's packed 16-bit per-lane counters; hpgv_set_cohort's own limit is lower). */
int  hpgv_assoc_model_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_counts8, void *stream);
/* d_counts8 (16-byte aligned) -> d_chisq5, d_p5: n_variants x 5 doubles each, [v * 5 + HPGV_MODEL_*] */
int  hpgv_assoc_model_stats_dev(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants, double *d_chisq5, double *d_p5,
                                void *stream);
/* d_gt in assoc layout, d_counts8 what hpgv_assoc_model_scan_dev wrote for it -> d_n_ge (n_variants int32), d_batch_max
 * (n_perms doubles), both overwritten.  d_perm_sums (may be NULL): {R_p, D_p} as int32[(v * n_perms + p) * 2 + k].
 * Alignment as hpgv_assoc_perm_dev: d_gt and d_counts8 16 bytes, d_batch_max and d_perm_sums 8.  Asynchronous on `stream`.
 * HPGV_ERR_STATE without labels.  The launch reads the genotype matrix ceil(n_perms / 128) times. */
int  hpgv_assoc_trend_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const int32_t *d_counts8,
                               int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_sums /* may be NULL */, void *stream);

/* ---- stratified association: the allelic test within the strata of a discrete stratification -- site, batch, ancestry
 *      cluster, matched set -- and the homogeneity of its odds ratio across them (PLINK's --mh / --bd with --within; no reference
 *      counterpart, and parity with PLINK is unpinned: this block is the specification).
 *
 *      Tables.  Stratum k of K has the 2 x 2 allele table a = A1_k, b = A2_k (affected), c = U1_k, d = U2_k (unaffected): the
 *      integers hpgv_assoc_scan_dev would count over that stratum's cohort columns alone, i.e. the sums of the contributions
 *      (c1, c2) of "label permutation" above -- with its chr-X rule for a row whose d_is_x is set -- over the stratum's affected
 *      and unaffected columns.  A missing call contributes nothing.  A column with a negative stratum or with HPGV_COND_OTHER is
 *      in no table.  tables[v * K + k] = {A1_k, A2_k, U1_k, U2_k} (int32 x 4), exact, from an i8 product on the matrix cores
 *      (csrc/hpgv_assoc_cmh_kernels.h).  Below m1 = a + b, m0 = c + d, n1 = a + c, n0 = b + d, n = m1 + m0, everything f64 without
 *      contraction, every sum over the strata in the order 0 .. K - 1.
 *
 *      CMH.  The strata with n >= 2 take part (n_strata_cmh of them).
 *          E_k = (m1 n1) / n,   V_k = ((m1 m0) (n1 n0)) / ((n n) (n - 1))
 *          chisq = (sum a - sum E)^2 / sum V      no continuity correction
 *      NaN -- never an infinity -- unless sum V > 0: a monomorphic row, a row with all calls missing, a row with no stratum taking
 *      part.  p = the 1-df tail by the device function hpgv_assoc_chisq_dev uses.
 *
 *      Mantel-Haenszel odds ratio, in the orientation of hpgv_assoc's odds (a d / (b c)), over the same strata:
 *          R_k = (a d) / n,   S_k = (b c) / n,   or_mh = sum R / sum S        NaN unless sum R > 0 and sum S > 0
 *      se of ln or_mh by Robins, Breslow and Greenland (1986): with P_k = (a + d) / n, Q_k = (b + c) / n
 *          se^2 = sum P R / (2 (sum R)^2) + sum (P S + Q R) / (2 (sum R)(sum S)) + sum Q S / (2 (sum S)^2)
 *          l95, u95 = exp(ln or_mh -/+ z se),   z = 1.959963984540054          all three NaN where or_mh is
 *
 *      Breslow-Day homogeneity of the odds ratio, without Tarone's correction.  A stratum enters when m1, m0, n1 and n0 are all
 *      positive (n_strata_bd of them).  With psi = or_mh the fitted count A_k is the root of
 *          (1 - psi) A^2 + qb A - psi m1 n1 = 0,   qb = (m0 - n1) + psi (m1 + n1)
 *      that lies in [max(0, n1 - m0), min(m1, n1)]: always the root with + sqrt(disc), disc = qb^2 + 4 (1 - psi) psi m1 n1.  It is
 *      evaluated in the form that does not cancel: for qb >= 0 as 2 psi m1 n1 / (qb + sqrt(disc)), for qb < 0 (which needs
 *      psi < 1) as (sqrt(disc) - qb) / (2 (1 - psi)); where |1 - psi| < 1e-12 by the linear equation, A_k = psi m1 n1 / qb.
 *          W_k = 1 / (1 / A + 1 / (m1 - A) + 1 / (n1 - A) + 1 / ((m0 - n1) + A))
 *          chisq_bd = sum (a - A_k)^2 / W_k,   df = n_strata_bd - 1
 *      NaN when df < 1, when or_mh is NaN, or when a fitted cell of an entered stratum is not positive.  p_bd = the upper chi-square
 *      tail for the integer df by the finite closed forms
 *          even df:  e^(-x/2) sum_{i < df/2} (x/2)^i / i!
 *          odd df :  erfc(sqrt(x/2)) + sqrt(2x/pi) e^(-x/2) sum_{i = 1 .. (df-1)/2} x^(i-1) / (1 . 3 ... (2i-1))
 *      each sum by its term recurrence from the smallest index; df = 1 is the 1-df tail above, bit for bit.  Where e^(-x/2)
 *      underflows (x above 1490) the tail is 0.
 *
 *      A row's record depends on that row only, and no step uses an atomic: a matrix passed in one call or in pieces, on any
 *      stream or device, gives identical bytes. */
enum { HPGV_CMH_MAX_STRATA = 1024 };
/* 72 bytes; arrays of it are 8-byte aligned */
typedef struct { int32_t n_strata_cmh, n_strata_bd; double chisq, p, or_mh, se, l95, u95, chisq_bd, p_bd; } hpgv_cmh_result;
/* stratum_of_sample[j] for VCF column j, the indexing of hpgv_set_cohort's condition[]: 0 .. n_strata - 1, or negative for "in no
 * stratum" (what a HPGV_COND_OTHER column holds is not read).  After hpgv_set_cohort (else HPGV_ERR_STATE); n_samples must be the
 * cohort's and a value >= n_strata in a cohort column is HPGV_ERR_INVALID; n_strata above HPGV_CMH_MAX_STRATA is
 * HPGV_ERR_UNSUPPORTED.  n_strata == 0 drops the strata; so does a new hpgv_set_cohort.  A group context gives every member the
 * strata.  The stratum image -- 2 n_strata rows rounded up to 16, of the assoc layout's pitch bytes: row 2k "stratum k and
 * affected", row 2k + 1 "stratum k and unaffected", in the label matrix's format -- is a buffer of its own (HPGV_ERR_NOMEM when it
 * does not fit): the labels of hpgv_set_perm_labels are untouched.  Not to be called while CMH calls of the context are in flight. */
int  hpgv_set_strata(hpgv_ctx *ctx, const int32_t *stratum_of_sample, int n_samples, int n_strata);
/* d_gt in assoc layout (16-byte aligned) -> d_out[v] (8-byte aligned) and d_tables (16-byte aligned; n_variants x n_strata x 4
 * int32; NULL: the context's own scratch, grown after `stream` has drained).  Two launches, asynchronous on `stream`: the tables
 * (the genotype matrix is read ceil(2 n_strata / 128) times), then one thread per variant for the record.  HPGV_ERR_STATE without
 * strata; HPGV_ERR_INVALID for n_variants < 0, a NULL or misaligned pointer. */
int  hpgv_assoc_cmh_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x /* may be NULL */,
                        hpgv_cmh_result *d_out, int32_t *d_tables /* may be NULL */, void *stream);
/* The same on a host batch in VCF column order (as hpgv_assoc_perm: chain stager, HPGV_LAYOUT_ASSOC layout, is_x per row or NULL)
 * and on a text (as hpgv_assoc_model_text: tokenizer, record filters, line status; a line that is not a record or that a record
 * filter rejected has its status set and its record and tables left as they were).  out: n_variants (max_lines) records; tables
 * (may be NULL): n_variants (max_lines) x n_strata x 4 int32.  Synchronous and thread-safe; a group context deals the call to a
 * member. */
int  hpgv_assoc_cmh(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x /* may be NULL */,
                    hpgv_cmh_result *out, int32_t *tables /* may be NULL */);
int  hpgv_assoc_cmh_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                         uint64_t *line_off, uint32_t *field_off, int32_t *status,
                         hpgv_cmh_result *out, int32_t *tables /* may be NULL */);
/* The definition on the host, by the function the statistics kernel compiles: tables = n_strata x {A1, A2, U1, U2}.  No GPU call,
 * no context.  HPGV_ERR_INVALID for n_strata < 0, a NULL pointer it needs, a negative count. */
int  hpgv_cmh_fit(const int32_t *tables, int n_strata, hpgv_cmh_result *out);
/*      Permutation within strata: max(T) empirical p-values of CHISQ_CMH (PLINK's --mh --mperm with --within).  Shuffling the
 *      labels across the whole cohort is the wrong null for a stratified test; here a labelling moves labels inside a stratum only
 *      (hpgv_perm_labels_shuffle_within makes such rows; the kernel itself takes any 0/1 rows).  Under a labelling y_p -- the rows
 *      of hpgv_set_perm_labels: same state, same limits, same rules for HPGV_COND_OTHER columns; a row need not keep the class
 *      sizes -- stratum k has the permuted counts
 *          a_p,k = sum_{j in stratum k} c1(v, j) y_p(j)      b_p,k = sum_{j in stratum k} c2(v, j) y_p(j)
 *          c_p,k = (A1_k + U1_k) - a_p,k                     d_p,k = (A2_k + U2_k) - b_p,k
 *      with (c1, c2) of "label permutation" and its chr-X rule and {A1_k, A2_k, U1_k, U2_k} the observed table above: exact
 *      integers, K i8 products on the matrix cores (csrc/hpgv_assoc_cmh_perm_kernels.h).  T_p(v) is chisq of the CMH paragraph on
 *      the K permuted tables -- the same strata rule (n >= 2), the same E_k and V_k expressions, f64 without contraction, sums over
 *      k = 0 .. K - 1 in that order, NaN unless sum V > 0 -- so it is bit for bit what hpgv_cmh_fit returns as chisq for those
 *      tables; T_obs(v) is the record's chisq.  No mean imputation and no variance held fixed: with missing calls m1_k changes
 *      with the labelling and is recomputed.  Outputs, NaN rules and merge rule are those of hpgv_assoc_perm_dev: n_ge[v],
 *      batch_max[p], element-wise maximum over batches, then hpgv_perm_pvalues.  They come from integer atomics and a maximum on
 *      the f64 bit pattern only: a matrix passed whole or in pieces, on any stream or device, gives identical bytes.
 *      Cost: only the 64-column steps of the assoc layout that hold a member of stratum k are multiplied for it.  Where every
 *      stratum is a contiguous block of layout columns the launch does about the matrix-core work of hpgv_assoc_perm_dev at the same
 *      n_perms; with fully interleaved strata up to n_strata times that.
 *      Not here: permutation of the Breslow-Day statistic, adaptive permutation, a layout sorted by stratum, a resident group form. */
/* d_gt in assoc layout, d_tables what hpgv_assoc_cmh_dev wrote for the same rows -> d_n_ge (n_variants int32), d_batch_max (n_perms
 * doubles), both overwritten.  d_perm_chisq (may be NULL): T_p(v) as double[v * n_perms + p].  d_gt and d_tables 16-byte aligned,
 * d_batch_max and d_perm_chisq 8-byte aligned.  Asynchronous on `stream`.  HPGV_ERR_STATE without strata or without labels;
 * HPGV_ERR_UNSUPPORTED for a grid over 2^31 - 1 workgroups (ceil(n_variants / 64) x ceil(n_perms / 64)): give the variants in
 * several calls.  The launch reads the genotype matrix at least ceil(n_perms / 64) times. */
int  hpgv_assoc_cmh_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x /* may be NULL */,
                             const int32_t *d_tables, int32_t *d_n_ge, double *d_batch_max, double *d_perm_chisq /* may be NULL */,
                             void *stream);
/* hpgv_assoc_cmh / hpgv_assoc_cmh_text plus the permutation's two outputs: out[v] is hpgv_assoc_cmh's record byte for byte, n_ge
 * (n_variants / max_lines int32) and batch_max (n_perms doubles) are overwritten.  A text line that is not a record or that a
 * record filter rejected takes no part in batch_max, gets n_ge 0 and has its record left as it was.  Synchronous and thread-safe;
 * a group context deals the call to a member (there is no resident group form). */
int  hpgv_assoc_cmh_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x /* may be NULL */,
                         hpgv_cmh_result *out, int32_t *n_ge, double *batch_max);
int  hpgv_assoc_cmh_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                              uint64_t *line_off, uint32_t *field_off, int32_t *status,
                              hpgv_cmh_result *out, int32_t *n_ge, double *batch_max);

/* ---- Logistic regression: the association test with covariates (PLINK's --logistic --covar; no reference counterpart, and
 *      parity with PLINK is unpinned: this block is the specification).  One regression per variant, of the phenotype on the
 *      ALT allele count and up to HPGV_LOGISTIC_MAX_COVAR covariates per sample -- the principal components of hpgv_pca_dev, say.
 *
 *      Observations of a row v in the assoc layout: the cohort columns whose genotype at v is not missing, by the byte rule of
 *      "model tests" above (missing / 0 / 1 / 2, "1/2" is hom-alt).  d = class index = number of ALT alleles; y = 1 for an
 *      affected column, 0 for an unaffected one.  Pad bytes are never observations.  Chromosome X gets no special rule.
 *
 *      Design row x = [1, d, c_1 .. c_C], p = C + 2 coefficients, 0 <= C <= HPGV_LOGISTIC_MAX_COVAR (so p <= 16).
 *
 *      Fit: Newton-Raphson from beta = 0, everything f64.  Per iteration, over the observations:
 *          eta = x . beta   (fma chain: beta_0, then i = 1 .. p - 1 in order)
 *          mu = 1 / (1 + exp(-eta)),   w = mu (1 - mu)
 *          H = sum w x x^T  (term (w x_i) x_j added with one fma),   u = sum (y - mu) x  (one fma per term)
 *      H = L L^T by Cholesky (right-looking, no pivoting); a pivot <= 1e-12 x the diagonal element of H it came from -- or a NaN
 *      one -- ends the fit as SINGULAR.  V = H^-1 = L^-T L^-1, the step delta_i = sum_j V_ij u_j (j ascending), beta += delta.
 *      Converged when max_i |delta_i| <= tol.  max_iter in 1 .. 100, tol finite and >= 0.
 *      The order in which the observations are summed is fixed per implementation (the device: hpgv_assoc_logistic_dev below;
 *      the host: index order), so results are reproducible; the two orders differ by rounding only.
 *
 *      Covariance: V of the H that produced the LAST step (no further pass over the samples).  se_i = sqrt(V_ii);
 *      stat = (beta_1 / se_1)^2 for the genotype coefficient; p = the 1-df chi-square tail by the device function
 *      hpgv_assoc_chisq_dev uses (the host form: the same expression on libm's erf / erfc).
 *
 *      Status per row:
 *          HPGV_LOGIT_OK             converged
 *          HPGV_LOGIT_NOT_CONVERGED  max_iter steps were taken without convergence, or a non-finite beta appeared
 *          HPGV_LOGIT_SINGULAR       the pivot rule above: a row monomorphic among its observations, d collinear with the
 *                                    intercept or a covariate, n_obs < p (n_obs = 0 included), and most separated data
 *      On any status but OK beta, se, stat and p are NaN; n_obs and iters (the steps taken, i.e. additions to beta) are
 *      still written. */
enum { HPGV_LOGISTIC_MAX_COVAR = 14 };
enum { HPGV_LOGIT_OK = 0, HPGV_LOGIT_NOT_CONVERGED = 1, HPGV_LOGIT_SINGULAR = 2 };
/* 48 bytes; arrays of it are 16-byte aligned.  beta, se: of the genotype coefficient (index 1) */
typedef struct { double beta, se, stat, p; int32_t n_obs, iters, status, pad; } hpgv_logistic_result;
/* cov[j * n_covar + k]: covariate k of VCF column j, the indexing of hpgv_set_cohort's condition[].  Kept on the device in the
 * assoc layout's column order, one row of pitch doubles per covariate, zeros under the pads.  After
 * hpgv_set_cohort (else HPGV_ERR_STATE); n_samples must be the cohort's (else HPGV_ERR_INVALID); n_covar above
 * HPGV_LOGISTIC_MAX_COVAR is HPGV_ERR_UNSUPPORTED; a non-finite value in a cohort column is HPGV_ERR_INVALID (columns with
 * HPGV_COND_OTHER may hold anything).  n_covar == 0 clears them; so does a new hpgv_set_cohort.  A group context gives every
 * member the covariates.  Not to be called while logistic calls of the context are in flight. */
int  hpgv_set_covariates(hpgv_ctx *ctx, const double *cov, int n_samples, int n_covar);
/* d_gt in assoc layout (16-byte aligned) -> d_out[v] (16-byte aligned) and, unless NULL, d_coef (8-byte aligned):
 * n_variants x 2p doubles, beta_0 .. beta_{p-1} then se_0 .. se_{p-1}, NaN on failure.  Without covariates C = 0.  One launch
 * runs the whole fit of every row; asynchronous on `stream`.  A row's results depend on that row only: one workgroup of four
 * waves per row, every lane sums its samples in position order, lanes are added by a fixed butterfly, waves in wave order, no
 * floating-point atomics -- a matrix passed in one call or in pieces gives bit-identical records, and so do two runs.
 * HPGV_ERR_INVALID for max_iter outside 1 .. 100, a tol that is negative or not finite, n_variants < 0, a NULL or
 * misaligned pointer. */
int  hpgv_assoc_logistic_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int max_iter, double tol,
                             hpgv_logistic_result *d_out, double *d_coef /* may be NULL */, void *stream);
/* The same on a host batch in VCF column order (as hpgv_assoc_model: chain stager, HPGV_LAYOUT_ASSOC layout) and on a text (as
 * hpgv_assoc_model_text: tokenizer, record filters, line status).  out: n_variants (max_lines) records; coef (may be NULL):
 * n_variants (max_lines) x 2p doubles.  Synchronous and thread-safe; a group context deals the call to a member. */
int  hpgv_assoc_logistic(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int max_iter, double tol,
                         hpgv_logistic_result *out, double *coef /* may be NULL */);
int  hpgv_assoc_logistic_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                              uint64_t *line_off, uint32_t *field_off, int32_t *status, int max_iter, double tol,
                              hpgv_logistic_result *out, double *coef /* may be NULL */);
/* The definition on the host, samples in index order: cls[i] in {0, 1, 2} or anything else for missing, y[i] 1 = affected,
 * cov[i * n_covar + k].  coef (may be NULL): 2p doubles.  No GPU call, no context.  HPGV_ERR_INVALID for n < 0, n_covar
 * outside 0 .. HPGV_LOGISTIC_MAX_COVAR, a bad max_iter or tol, a NULL pointer it needs. */
int  hpgv_logistic_fit(const uint8_t *cls, const uint8_t *y, const double *cov, int n, int n_covar, int max_iter, double tol,
                       hpgv_logistic_result *out, double *coef /* may be NULL */);

/* ---- Linear regression: the association test of a quantitative trait with covariates (PLINK's --linear --covar; no reference
 *      counterpart, and parity with PLINK is unpinned: this block is the specification).  One ordinary least squares fit per
 *      variant, of the trait y on the ALT allele count and up to HPGV_LOGISTIC_MAX_COVAR covariates per sample.
 *
 *      Observations of a row v, the byte rule and the class d in {0, 1, 2}: those of "Logistic regression" above.  Both segments
 *      of the assoc layout are cohort columns (the condition only places a column); pads are never observations; chromosome X
 *      gets no special rule.  y is a finite double per cohort column (hpgv_set_phenotype).
 *
 *      Design row x = [1, d, c_1 .. c_C], p = C + 2.  Everything f64:
 *          beta = (X^T X)^-1 X^T y,   RSS = y^T y - |L^-1 X^T y|^2 with X^T X = L L^T,   df = n_obs - p,   sigma^2 = RSS / df,
 *          se_i = sqrt(sigma^2 V_ii) with V = (X^T X)^-1,   stat = beta_1 / se_1 (a signed t statistic),
 *          p = the two-sided Student-t tail with df degrees of freedom (hpgv_linear_t_p).
 *
 *      Moments by class sums -- the device kernel and the host fit use the same identity.  f_s = [1, c_1 - m_1, .., c_C - m_C,
 *      y - m_y] is the feature row of cohort column s (q = C + 2 entries); the means m and G = sum_cohort f f^T are taken over
 *      the cohort columns in layout order (the host fit: index order) once per set call, one fma per term.  For a row:
 *          h = sum_obs d_s f_s (the dense product),   n_1, n_2 the class counts,   n_miss, n_obs
 *          dd = n_1 + 4 n_2,   sum_obs d = n_1 + 2 n_2 (both exact, from the integers)
 *          S = G - sum_missing f f^T  when n_miss <= n_obs,   S = sum_obs f f^T  otherwise
 *      either sum over its positions in ascending order, one fma per term.  The normal equations in the order [1, d, c ..] are
 *      read off S, h and dd; y^T y = S[y][y]; X^T y is the y column of S and h[y] for d.  Cholesky and inverse as in the logistic
 *      fit (same function, same pivot rule).  The centring is internal; the reported intercept is transformed back:
 *          beta_0 = beta'_0 + m_y - sum_k beta_k m_k,   se_0 = sqrt(sigma^2 a^T V a) with a = (1, 0, -m_1, .., -m_C).
 *
 *      Status per row:
 *          HPGV_LINEAR_OK
 *          HPGV_LINEAR_SINGULAR  the pivot rule fired or df < 1: all-missing and monomorphic rows, d collinear with a covariate,
 *                                n_obs <= p.  All doubles are NaN.
 *          HPGV_LINEAR_EXACT     RSS <= 1e-12 S[y][y]: a perfect fit.  beta is written, se = 0, stat and p are NaN.
 *      n_obs and df are always written. */
enum { HPGV_LINEAR_OK = 0, HPGV_LINEAR_SINGULAR = 1, HPGV_LINEAR_EXACT = 2 };
/* 48 bytes; arrays of it are 16-byte aligned.  beta, se: of the genotype coefficient (index 1) */
typedef struct { double beta, se, stat, p; int32_t n_obs, df, status, pad; } hpgv_linear_result;
/* y[j]: the trait of VCF column j, the indexing of hpgv_set_cohort's condition[].  After hpgv_set_cohort (else HPGV_ERR_STATE);
 * n_samples must be the cohort's (else HPGV_ERR_INVALID); a non-finite value in a cohort column is HPGV_ERR_INVALID (columns
 * with HPGV_COND_OTHER may hold anything).  y == NULL clears the phenotype; so does a new hpgv_set_cohort.  A group context
 * gives every member the phenotype.  This call and hpgv_set_covariates each rebuild the linear model's device image while a
 * phenotype is set: the centred features, sample-major, 16 doubles per layout position (zeros under pads and in unused
 * columns), then G and the means.  Not to be called while linear calls of the context are in flight. */
int  hpgv_set_phenotype(hpgv_ctx *ctx, const double *y, int n_samples);
/* d_gt in assoc layout (16-byte aligned) -> d_out[v] (16-byte aligned) and, unless NULL, d_coef (8-byte aligned):
 * n_variants x 2p doubles, beta_0 .. beta_{p-1} then se_0 .. se_{p-1} (NaN when SINGULAR; se 0 when EXACT).  One launch,
 * asynchronous on `stream`: a workgroup of four waves owns 16 rows, h is their product with the feature image on
 * v_mfma_f64_16x16x4_f64 (the waves take the positions in a fixed pattern and are added in wave order), the counts are
 * integers, the correction of S walks a row's flagged positions in ascending order, no floating-point atomics.  A row's record
 * depends on that row only: a matrix passed in one call or in pieces gives bit-identical records, and so do two runs.
 * HPGV_ERR_STATE without a cohort or without a phenotype; HPGV_ERR_INVALID for n_variants < 0, a NULL or misaligned pointer. */
int  hpgv_assoc_linear_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, hpgv_linear_result *d_out,
                           double *d_coef /* may be NULL */, void *stream);
/* The same on a host batch in VCF column order and on a text, built as hpgv_assoc_logistic and hpgv_assoc_logistic_text are.
 * Synchronous and thread-safe; a group context deals the call to a member. */
int  hpgv_assoc_linear(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, hpgv_linear_result *out,
                       double *coef /* may be NULL */);
int  hpgv_assoc_linear_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                            uint64_t *line_off, uint32_t *field_off, int32_t *status, hpgv_linear_result *out,
                            double *coef /* may be NULL */);
/* The definition on the host, samples in index order (every one of the n samples is a cohort column): cls[i] in {0, 1, 2} or
 * anything else for missing, y[i], cov[i * n_covar + k].  coef (may be NULL): 2p doubles.  No GPU call, no context.
 * HPGV_ERR_INVALID for n < 0, n_covar outside 0 .. HPGV_LOGISTIC_MAX_COVAR, a NULL pointer it needs, a y or covariate that is
 * not finite. */
int  hpgv_linear_fit(const uint8_t *cls, const double *y, const double *cov, int n, int n_covar, hpgv_linear_result *out,
                     double *coef /* may be NULL */);
/* The two-sided tail of Student's t with df degrees of freedom at t: I_x(df / 2, 1 / 2) with x = df / (df + t^2), the
 * regularised incomplete beta function by its continued fraction (through the complement 1 - I_{1 - x}(1 / 2, df / 2) where x
 * is large).  NaN for a NaN t or df < 1.  The function the kernel compiles too. */
double hpgv_linear_t_p(double t, int df);

/* ---- permutations of the linear statistic: max(T) empirical p-values of the quantitative-trait regression (PLINK's --linear
 *      --mperm; no reference counterpart, and parity with PLINK is unpinned: this block is the specification).
 *
 *      Cohort columns, the byte rule, the dosage d in {0, 1, 2} and the design [1, d, c_1 .. c_C] are those of "Linear regression".
 *      N = the number of cohort columns, p = C + 2, df = N - p for every row: missing calls are imputed by the row's mean dosage.
 *      The reduced model's fitted values stay in place and its residuals are permuted (Freedman and Lane 1983).
 *
 *      Once per hpgv_set_linear_perms, on the host, in f64, over the cohort positions in layout order (the host fit: index
 *      order), every dot product one fma per term:
 *          Q_1 .. Q_C   an orthonormal basis of the centred covariates by modified Gram-Schmidt in column order: column k, centred
 *                       by its mean, loses Q_j (Q_j . v) for j = 1 .. k - 1 one after the other, v what the earlier steps left, and
 *                       is scaled to length 1.  A column whose remaining squared norm is <= 1e-12 x its centred squared norm makes
 *                       the covariates collinear: HPGV_ERR_INVALID.
 *          e            = y - m_y with Q_1 .. Q_C taken out the same way: the residual of the reduced model.  ss_0 = e . e.
 *          eps_p(j)     = e(order_p(j)) for permutation p of the cohort columns.
 *          E_p          = eps_p - mean(eps_p) with Q_1 .. Q_C taken out the same way.  ss_p = E_p . E_p.
 *      Per row v, O its observed cohort positions, n_obs, n_1, n_2 its integer class counts:
 *          mu = (n_1 + 2 n_2) / n_obs,   w_s = d_s - mu on O and 0 on a missing call (the mean-imputed, centred dosage),
 *          sw2 = (n_1 + 4 n_2) - n_obs mu^2,   D = sw2 - sum_k (sum_O d Q_k - mu sum_O Q_k)^2.
 *          The row takes no part if n_obs = 0, sw2 <= 0, D <= 1e-12 sw2 or df < 1: t_obs = NaN, n_ge = 0, never in a maximum.
 *      Per (v, p):
 *          u = sum_O d E_p - mu sum_O E_p  (two products, over the dosage plane and the valid plane),   r2 = u^2 / (D ss_p),
 *          T_p = sign(u) sqrt(df r2 / (1 - r2)) when r2 < 1 - 1e-12, else NaN (a NaN r2 gives NaN).
 *      T_obs is the same function of e and ss_0.  |T| is what is compared and what enters the maxima.
 *
 *      For a row without missing calls T_obs equals hpgv_assoc_linear's stat up to rounding (Frisch-Waugh-Lovell).  For a row with
 *      missing calls T_obs is the statistic of the mean-imputed row, NOT of the observed subset that hpgv_assoc_linear fits: an
 *      exact refit per subset needs a p x p solve per (row, permutation), while under imputation the projection is shared by all
 *      rows and a (row, permutation) costs two dot products whatever C is -- the whole scan is one f64 matrix product.  Mean
 *      imputation is what hpgv_score does with a missing call.
 *
 *      Outputs per call, by the rules of hpgv_assoc_perm_dev: t_obs[v]; n_ge[v] = #{p : |T_p| >= |T_obs|}; batch_max[p] = max_v
 *      |T_p(v)| over the rows that take part (0.0 when none does; a NaN never enters).  Batches merge by the element-wise maximum;
 *      then hpgv_perm_pvalues with |t_obs|. */
/* Host only.  order_out[p * n_samples + j] = the VCF column whose residual column j takes under permutation p: the counter-based
 * SplitMix64 keys and the Fisher-Yates walk of hpgv_perm_labels_shuffle over the list of cohort columns in VCF order (row p does
 * not depend on n_perms).  HPGV_COND_OTHER columns map to themselves. */
int  hpgv_perm_order_shuffle(const uint8_t *condition, int n_samples, int n_perms, uint64_t seed, int32_t *order_out);
/* order: n_perms rows of n_samples columns as hpgv_perm_order_shuffle writes them (what a row holds in HPGV_COND_OTHER columns is
 * not read).  After hpgv_set_cohort and hpgv_set_phenotype (else HPGV_ERR_STATE).  A row that is not a bijection of the cohort
 * columns and collinear covariates are HPGV_ERR_INVALID; more than 1 048 576 permutations HPGV_ERR_UNSUPPORTED; an image that does
 * not fit the device HPGV_ERR_NOMEM.  n_perms == 0 drops the permutations; so do hpgv_set_phenotype, hpgv_set_covariates and
 * hpgv_set_cohort.  A group context gives every member the permutations.  The device image has the layout of the linear model's
 * features in tiles of 16 columns -- [tile][position][16 doubles], positions rounded up to 64, zeros under pads: tile 0 holds
 * Q_1 .. Q_C and e, tile 1 + p / 16 holds E_p in column p % 16 -- with ss_0, ss_1 .. behind it. */
int  hpgv_set_linear_perms(hpgv_ctx *ctx, const int32_t *order, int n_perms);
/* d_gt in assoc layout (16-byte aligned) -> d_t_obs[v], d_n_ge[v], d_batch_max[p] (8-byte aligned) and, unless NULL, d_perm_t
 * [v * n_perms + p] (8-byte aligned): every T_p(v), NaN where the definition says so.  Two launches, asynchronous on `stream`: the
 * row pass (mu, D, T_obs per row) and the product of 64 rows x 128 permutations per workgroup on v_mfma_f64_16x16x4_f64.  The sum
 * over the positions has a fixed order and integer atomics alone merge the workgroups: T_p(v) depends on row v only, a matrix
 * passed whole or in pieces gives bit-identical d_perm_t, and so do two runs.  Not to be called on two streams at once (the row
 * pass's scratch is the context's).  HPGV_ERR_STATE without a cohort, a phenotype or permutations; HPGV_ERR_INVALID for
 * n_variants < 0, a NULL or misaligned pointer. */
int  hpgv_assoc_linear_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, double *d_t_obs, int32_t *d_n_ge,
                                double *d_batch_max, double *d_perm_t /* may be NULL */, void *stream);
/* The same on a host batch in VCF column order and on a text, built as hpgv_assoc_perm and hpgv_assoc_perm_text are; out[v]: the
 * hpgv_assoc_linear record of the same row.  A line of a text that is no record or that a record filter rejects takes no part.
 * batch_max is written for n_variants == 0 too.  Synchronous and thread-safe; a group context deals the call to a member. */
int  hpgv_assoc_linear_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, hpgv_linear_result *out,
                            double *t_obs, int32_t *n_ge, double *batch_max);
int  hpgv_assoc_linear_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                                 uint64_t *line_off, uint32_t *field_off, int32_t *status, hpgv_linear_result *out,
                                 double *t_obs, int32_t *n_ge, double *batch_max);
/* The definition on the host, samples in index order (every one of the n samples is a cohort column), for one row: cls, y and cov
 * as hpgv_linear_fit takes them, order[p * n + j] the sample whose residual sample j takes -> *t_obs and t_perm[p].  It compiles
 * the functions the kernels compile: row scalars -> D, and (u, D, ss, df) -> T.  No GPU call, no context.  HPGV_ERR_INVALID for
 * what hpgv_linear_fit refuses, an order row that is no bijection of 0 .. n - 1, collinear covariates. */
int  hpgv_linear_perm_fit(const uint8_t *cls, const double *y, const double *cov, int n, int n_covar, const int32_t *order,
                          int n_perms, double *t_obs, double *t_perm);

/* d_gt in tdt layout -> d_tu[v] = {t1, t2} (int32 x2) */
int  hpgv_tdt_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants,
                       const uint8_t *d_is_x, int32_t *d_tu, void *stream);
int  hpgv_tdt_stats_dev(hpgv_ctx *ctx, const int32_t *d_tu, int n_variants,
                        double *d_odds, double *d_chisq, double *d_p, void *stream);

/* ---- family flips of the TDT: max(T) empirical p-values (PLINK's tdt --mperm; no reference counterpart).  Shuffling labels is
 *      the wrong null for the TDT; its permutation flips "transmitted" and "untransmitted" for every child of a family at once,
 *      with probability 1/2 per family and permutation.  Family f contributes (t1_f, t2_f) to a variant's {t1, t2}
 *      (tdt.c:175-239); flipped it contributes (t2_f, t1_f).  Under the signs s_p(f) = +1 (kept) / -1 (flipped)
 *          t1_p + t2_p = t1 + t2 = n,       t1_p - t2_p = D_p = sum_f s_p(f) d_f,   d_f = t1_f - t2_f
 *      so {t1_p, t2_p} = {(n + D_p) / 2, (n - D_p) / 2}, integral because t1_f + t2_f and t1_f - t2_f have the same parity: one i8
 *      matrix product over the families with exact i32 sums on the matrix cores (csrc/hpgv_tdt_perm_kernels.h; K = the family
 *      count, a third of the TDT row).  T_p(v) is the chi-square of {t1_p, t2_p} by the device function hpgv_tdt_stats_dev uses,
 *      T_obs(v) the same on the observed counts.  A variant with t1 + t2 == 0 (chi-square -1) takes no part.  Outputs per call:
 *          n_ge[v]      = #{p : T_p(v) >= T_obs(v)}  (int32; 0 when t1 + t2 == 0)
 *          batch_max[p] = max over the call's variants of T_p(v)  (0.0 when no variant takes part)
 *      Calls are stateless and merge as the label permutation's do: batch_max by element-wise maximum, then hpgv_perm_pvalues,
 *      with NaN as t_obs for a variant whose chi-square is -1.  The resident sharded scan (hpgv_group_tdt) has no permutation form. */
/* flips[p * n_families + f] in {0, 1} (1 = flipped) for family f of hpgv_set_families, one row per permutation; families the plan
 * skips (a parent that is no column, no children) are ignored.  After hpgv_set_families (else HPGV_ERR_STATE); a group context
 * gives every member the flips.  n_perms == 0 drops the flips; so does a new hpgv_set_families.  A value above 1 under a counted
 * family: HPGV_ERR_INVALID.  Limits: more than 1 048 576 permutations per call, or a family with more than 63 counted children
 * (|d_f| <= 2 x children must fit i8), is HPGV_ERR_UNSUPPORTED; the sign matrix takes (n_perms rounded up to 16) x (fast trios
 * and slow families, each rounded up to 16) bytes of device memory and HPGV_ERR_NOMEM is returned when they are not there.  Not
 * to be called while permutation calls of the context are in flight. */
int  hpgv_set_tdt_flips(hpgv_ctx *ctx, const uint8_t *flips, int n_perms);
/* d_gt in tdt layout, d_tu what hpgv_tdt_scan_dev wrote for it -> d_n_ge (n_variants int32), d_batch_max (n_perms doubles), both
 * overwritten.  d_perm_tu (may be NULL; for tests and for callers who want another statistic): {t1_p, t2_p} as
 * int32[(v * n_perms + p) * 2 + k].  d_gt 16-byte aligned, d_tu, d_batch_max and d_perm_tu 8-byte aligned.  Asynchronous on
 * `stream`.  HPGV_ERR_STATE without flips.  With families of several children the call keeps their per-row differences in
 * scratch of the context: such calls of one context go on one stream.  The launch reads the genotype matrix ceil(n_perms / 128)
 * times, the passes of a row close together in time; ceil(n_variants / 512) x 8 x ceil(n_perms / 128) above 2^31 - 1 is
 * HPGV_ERR_UNSUPPORTED (give the variants in several calls). */
int  hpgv_tdt_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_tu,
                       int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_tu /* may be NULL */, void *stream);

/* d_gt in stats layout -> per variant 8 x int32:
 *   {n_00, n_01, n_10, n_11, missing_genotypes, missing_alleles, allele0, allele1}
 * (biallelic cells of genotypes_count[a1*2+a2]; allele counts include the called
 * allele of half-missing genotypes; genotypes touching an allele index >= 2 are
 * n_samples - missing_genotypes - the four cells) and Hardy-Weinberg chi2 / p on
 * (n_00, n_01+n_10, n_11). */
int  hpgv_stats_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants,
                         int32_t *d_counts8, void *stream);
int  hpgv_stats_hwe_dev(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants,
                        double *d_chi2, double *d_p, void *stream);
/* the same counters restricted to one phenotype group; d_gt in the HPGV_LAYOUT_STATS_GROUPS layout */
int  hpgv_stats_scan_group_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int group,
                               int32_t *d_counts8, void *stream);

/* per-sample missing-genotype counts (get_sample_stats, call site stats_runner.c:197-198) over a
 * stats-layout matrix: d_missing[j] += number of listed variants in which sample j has a missing
 * allele.  The caller zeroes d_missing (n_samples ints) before the first batch. */
int  hpgv_sample_missing_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants,
                             int32_t *d_missing, void *stream);

/* full genotype table of (multi-allelic) variants from a RAW HPGV8 matrix in VCF column order:
 * d_table[i*256 + code] = samples of variant d_variant_idx[i] (or variant i when NULL) whose
 * code byte is `code`; genotypes_count[a1*num_alleles + a2] is d_table[i*256 + (a1<<4|a2)]. */
int  hpgv_genotype_table_dev(hpgv_ctx *ctx, const uint8_t *d_raw, size_t src_pitch, int n_samples,
                             const int32_t *d_variant_idx, int n_idx, int32_t *d_table, void *stream);

/* d_gt in the HPGV_LAYOUT_MENDEL layout -> d_errors[v] = trios with a Mendelian error at variant v */
int  hpgv_mendel_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x,
                          int32_t *d_errors, void *stream);
/* d_child_errors[t] += variants at which trio t (order of hpgv_set_pedigree) has a Mendelian error;
 * the caller zeroes the n_trios counters before the first batch */
int  hpgv_mendel_children_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x,
                              int32_t *d_child_errors, void *stream);

/* count-derived variant filters (--maf, --missing of shared_options.c:42-47,86-115) from the stats
 * counters: d_keep[i] = 1 iff maf >= min_maf, maf <= max_maf and missing rate <= max_missing, where a
 * negative threshold switches that test off; maf = min(allele0, allele1) / (allele0 + allele1),
 * missing rate = missing_genotypes / n_samples of the stats cohort. */
int  hpgv_stats_filter_dev(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants,
                           double min_maf, double max_maf, double max_missing,
                           uint8_t *d_keep, void *stream);

/* the counts behind the inheritance filters (--inh-dom / --inh-rec, shared_options.c:42-56): d_gt in the
 * HPGV_LAYOUT_ASSOC layout -> per variant 8 x int32
 *   {c0 affected calls counted, c1 affected calls with a non-reference allele (byte != 0x00), c2 affected calls with
 *    both alleles non-reference, c3 unaffected calls counted, c4 unaffected calls 0/0 (byte == 0x00), c5 unaffected
 *    calls with both alleles non-reference, 0, 0}
 * A call is counted when neither allele nibble is 0xF (missing and half-missing genotypes are not); multi-allelic codes
 * count by the same rules.  Exact for any class size the cohort takes.  Needs hpgv_set_cohort (else HPGV_ERR_STATE);
 * d_gt and d_counts8 16-byte aligned.  Asynchronous on `stream`. */
int  hpgv_inheritance_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_counts8, void *stream);

/* ---- LD: the squared genotype correlation r^2 between variants that lie near each other (PLINK's --r2 --ld-window; no
 *      reference counterpart): what clumping, pruning and the annotation of a hit with its neighbours start from.
 *
 *      The genotype class of an HPGV8 byte is the model tests' ("model tests" above): missing if either nibble is 0xF, else
 *      0, 1 or 2 ("1/2" is 2); dosage equals class.  Chromosome X gets no special rule.  For rows a < b of one matrix, with
 *      v = valid (0 / 1) and g = dosage (0 when missing), summed over the row's bytes:
 *          n   = sum v_a v_b        sa  = sum g_a v_b        sb  = sum v_a g_b
 *          saa = sum g_a^2 v_b      sbb = sum v_a g_b^2      sab = sum g_a g_b
 *      the moments over the samples called in BOTH rows: six i8 products (planes v, g, g^2) with exact i32 sums on the matrix
 *      cores (csrc/hpgv_ld_kernels.h).  counts6 = {n, sa, sb, saa, sbb, sab}, int32 x 6.
 *
 *      Statistic.  The three differences in int64 (exact: the largest, n saa, stays below 2^47 for any row the layouts
 *      allow), the rest f64 without contraction, in this order:
 *          cov = n sab - sa sb      va = n saa - sa^2      vb = n sbb - sb^2
 *          r2  = ((double)cov * (double)cov) / ((double)va * (double)vb)
 *      va == 0 or vb == 0 gives 0 / 0 = NaN: a monomorphic row, n = 0 and n = 1.  Nothing else is special-cased, as the
 *      chi-square path special-cases no zero margin.  The sign of r is the sign of cov, which counts6 gives.
 *
 *      Band.  With `window` W the outputs are indexed by the LATER variant: r2[(b - b_begin) * W + (d - 1)] is the pair
 *      (b - d, b) for d = 1 .. W and b = b_begin .. n_variants - 1; counts6 uses the same index x 6.  Every element of that
 *      range is written.  A pair gets r2 = NaN and zero counts (it is "outside the band") when b - d < 0, when either row is
 *      skipped, when chromosomes are given and the two differ, or when positions are given, max_bp >= 0 and
 *      |pos_b - pos_a| > max_bp.  Only whether an r2 is NaN is defined, not which NaN. */
#define HPGV_LD_MAX_WINDOW 1024
/* d_gt: any matrix of HPGV8 rows `pitch` bytes apart whose pad bytes are 0xFF -- a matrix in the assoc layout is one, and the LD
 * is then over the cohort columns.  Rows below b_begin serve as earlier partners only: a caller that walks a file in pieces
 * prepends the last `window` rows of the previous piece and passes b_begin = window, which makes the seam exact without any
 * engine state.  d_chrom (int32 per row) and d_pos (uint32 per row): both or both NULL (else HPGV_ERR_INVALID); max_bp < 0
 * = no distance limit.  d_skip (may be NULL): != 0 = the row takes no part.  d_r2: (n_variants - b_begin) x window doubles;
 * d_counts6 (may be NULL) x 6 int32.  Needs no cohort.  n_variants == b_begin succeeds and writes nothing.
 * Refusals: window outside 1 .. HPGV_LD_MAX_WINDOW is HPGV_ERR_UNSUPPORTED (the passes of a tile grow with it), and so is a
 * call whose (n_variants / 64) x (window / 64 + 2) exceeds 2^31 workgroups; HPGV_ERR_INVALID for b_begin outside
 * 0 .. n_variants, a pitch that is 0, not a multiple of 16 or 4 GiB and more, d_gt not 16-byte aligned, d_r2 or d_counts6 not
 * 8-byte aligned, d_chrom or d_pos not 4-byte aligned.  Asynchronous on `stream`; under option "profile" its time is the
 * statistics time of hpgv_last_kernel_ms.  The launch reads each row window / 64 + 2 times at most, from L2 but for the first. */
int  hpgv_ld_window_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window,
                        const int32_t *d_chrom /* may be NULL */, const uint32_t *d_pos /* may be NULL */, int64_t max_bp,
                        const uint8_t *d_skip /* may be NULL */, double *d_r2, int32_t *d_counts6 /* may be NULL */, void *stream);
/* The EDGE form of the band: the same tile and loop with another epilogue (k_ld_edges, a kernel of its own), for a consumer that wants only the pairs
 * above a threshold (PLINK's --clump-r2, --ld-window-r2) and would discard nearly all of a dense band.  The result is exactly the
 * set {(a, b, r2) : a = b - d, r2 >= min_r2} over the band hpgv_ld_window_dev writes for the same arguments, r2 bit for bit the
 * value written there.  NaN never compares >=, so no pair "outside the band" appears, and none without an earlier row.  The
 * ORDER of the list is not defined (sort it where an order is needed).
 * The call zeroes *d_n_edges itself on `stream`; it ends as the TRUE number of qualifying pairs even where that exceeds edge_cap.
 * At most edge_cap records are stored and nothing past them; which of the qualifying pairs those are is not defined.
 * edge_cap == 0 with d_edges == NULL is a legal count-only call.  Per wave and (16 x 16 block, register) the qualifying lanes are
 * counted by ballot and claim their places with ONE relaxed 64-bit add; a record goes out as one 16-byte store.
 * Refusals and alignment as hpgv_ld_window_dev (d_r2 aside); also HPGV_ERR_INVALID for a NaN min_r2, d_edges not 16-byte
 * aligned or NULL with edge_cap > 0, d_n_edges NULL or not 8-byte aligned.  n_variants == b_begin succeeds with a count of 0. */
typedef struct { int32_t a, b; double r2; } hpgv_ld_edge;   /* 16 bytes, a < b */
int  hpgv_ld_edges_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window,
                       const int32_t *d_chrom /* may be NULL */, const uint32_t *d_pos /* may be NULL */, int64_t max_bp,
                       const uint8_t *d_skip /* may be NULL */, double min_r2, hpgv_ld_edge *d_edges, uint64_t edge_cap,
                       uint64_t *d_n_edges, void *stream);

/* ---- IBS: pairwise identity-by-state counts between SAMPLES and the relatedness estimates made of them (PLINK's --genome; no
 *      reference counterpart): duplicates, undeclared relatives and sample swaps, the first QC step of a cohort.  Parity with
 *      PLINK is UNPINNED, as Fisher's is: no PLINK was at hand, and the formulas below are this project's definition.
 *
 *      The genotype class g of an HPGV8 byte is LD's ("LD" above): missing if either nibble is 0xF, else the number of non-zero
 *      nibbles, 0, 1 or 2 ("1/2" is 2); pad bytes are 0xFF.  For byte COLUMNS i < j of one matrix, summed over the rows that are
 *      not skipped and where both columns are called:
 *          n = rows where both are called      ibs0 = rows with |g_i - g_j| = 2      ibs2 = rows with g_i = g_j
 *          ibs1 = n - ibs0 - ibs2
 *      The contraction runs over the ROWS of the variant-major matrix: four i8 products with exact i32 sums on the matrix cores
 *      (csrc/hpgv_ibs_kernels.h).  With the planes v = valid, h = [g = 1], m = v - h and s = g - 1 on valid bytes (else 0):
 *          P1 = s.s   P2 = m.m   P3 = h.h   P4 = v.v      ibs0 = (P2 - P1) / 2   ibs2 = (P2 + P1) / 2 + P3   n = P4
 *
 *      Expected IBS under IBD (method of moments).  Per row, over the columns: the class counts n0, n1, n2;
 *      X = 2 n0 + n1, Y = n1 + 2 n2, T = X + Y.  A row is USED iff it is not skipped and T >= 4.  fall(x, k) =
 *      x (x - 1) ... (x - k + 1), x converted to double first, the factors multiplied left to right, fall(x, 0) = 1;
 *      F(a, b) = (fall(X, a) * fall(Y, b)) / fall(T, a + b), the unbiased estimate of p^a q^b when drawing without replacement.
 *      The terms of a row, in this operation order:
 *          t00 = 2 F(2,2)                          t01 = 4 F(3,1) + 4 F(1,3)        t02 = (F(4,0) + F(0,4)) + 4 F(2,2)
 *          t11 = 2 F(2,1) + 2 F(1,2)               t12 = ((F(3,0) + F(0,3)) + F(2,1)) + F(1,2)
 *      E = {E00, E01, E02, E11, E12}: the sums of the terms over the used rows, added sequentially in file order in f64, divided
 *      by the number of used rows.
 *
 *      Per pair, f64 without contraction, in this order, S = (double)n:
 *          z0 = ibs0 / (E00 S)      z1 = (ibs1 - z0 (E01 S)) / (E11 S)      z2 = (ibs2 - z0 (E02 S) - z1 (E12 S)) / S
 *          clamps, in sequence:           z0 > 1: (1, 0, 0);   z1 > 1: (0, 1, 0);   z2 > 1: (0, 0, 1)
 *          renormalisations, in sequence: z0 < 0: t = z1 + z2, z1 /= t, z2 /= t, z0 = 0; the same for z1 < 0 over z0 and z2;
 *                                         the same for z2 < 0 over z0 and z1
 *          PI_HAT = z1 / 2 + z2      DST = ((double)ibs2 + 0.5 (double)ibs1) / S
 *      Nothing else is special-cased: n = 0 or a zero E give the IEEE NaN or inf that flow through these steps.  Only WHETHER a
 *      value is NaN is defined, not which NaN.
 *
 *      Out of scope: PLINK's PPC and RATIO columns, its re-projection of (z0, z1, z2) onto the "biologically plausible" region,
 *      and a group form of the batch calls. */
typedef struct { int32_t n, ibs0, ibs1, ibs2; } hpgv_ibs_counts;                       /* 16 bytes */
typedef struct { int32_t i, j; hpgv_ibs_counts c; double pi_hat; } hpgv_ibs_pair;      /* 32 bytes, i < j */
/* d_gt: any matrix of HPGV8 rows `pitch` bytes apart; the bytes of a row at and past n_cols are never counted, whatever they
 * hold.  d_skip (may be NULL): != 0 = the row takes no part.  The call ADDS the counts of these rows to d_counts[i * n_cols + j]
 * for 0 <= i < j < n_cols with relaxed device-scope atomics -- calls on pieces of a matrix, on several streams and from several
 * threads accumulate into one buffer -- and never touches any other element.  The caller zeroes the n_cols x n_cols records
 * (hpgv_memset_dev) before the first call and keeps the rows accumulated into one buffer below 2^31.  Needs no cohort.
 * n_variants == 0 or n_cols < 2 succeed and write nothing.  Refusals: HPGV_ERR_INVALID for n_variants < 0, n_cols < 0 or
 * n_cols > pitch, a pitch that is 0, not a multiple of 16 or 4 GiB and more, d_gt or d_counts not 16-byte aligned;
 * HPGV_ERR_UNSUPPORTED where ceil(n_cols / 64)^2 / 2 tile pairs times the row ranges exceed 2^31 workgroups.  Asynchronous on
 * `stream`; under option "profile" its time is the statistics time of hpgv_last_kernel_ms.  A launch reads the matrix
 * ceil(n_cols / 64) times, from L2 where the workgroups of an XCD share their rows. */
int  hpgv_ibs_pairs_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols,
                        const uint8_t *d_skip /* may be NULL */, hpgv_ibs_counts *d_counts /* n_cols x n_cols */, void *stream);
/* d_class4[4 * row + k] = {n0, n1, n2, missing} of the row over the columns below n_cols, zeros for a skipped row: every
 * element written, one wave per row.  Matrix, refusals and alignment as hpgv_ibs_pairs_dev (d_class4 16-byte aligned). */
int  hpgv_ibs_class_counts_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols,
                               const uint8_t *d_skip /* may be NULL */, int32_t *d_class4, void *stream);
/* The pairs of a counts matrix with PI_HAT >= min_pi_hat, hpgv_ld_edges_dev's contract: exactly the set {i < j : PI_HAT >=
 * min_pi_hat} with pi_hat bit for bit hpgv_ibs_genome's; NaN never compares >=, so a pair with a NaN PI_HAT never appears.  The
 * ORDER of the list is not defined.  The call zeroes *d_n itself on `stream`; it ends as the TRUE number of qualifying pairs
 * even where that exceeds cap.  At most cap records are stored and nothing past them; cap == 0 with d_pairs == NULL is a legal
 * count-only call.  Per wave the qualifying lanes are counted by ballot and claim their places with ONE relaxed 64-bit add.
 * HPGV_ERR_INVALID for a NaN min_pi_hat, n_cols < 0, a NULL E or d_n, d_pairs NULL with cap > 0, d_counts or d_pairs not 16-byte
 * aligned, d_n not 8-byte aligned; HPGV_ERR_UNSUPPORTED for n_cols x ceil(n_cols / 256) above 2^31 - 1. */
int  hpgv_ibs_select_dev(hpgv_ctx *ctx, const hpgv_ibs_counts *d_counts, int n_cols, const double E[5], double min_pi_hat,
                         hpgv_ibs_pair *d_pairs, uint64_t cap, uint64_t *d_n, void *stream);

/* ---- GRM: the genetic relationship matrix between SAMPLES (GCTA's --make-grm, PLINK's --make-grm-bin; no reference
 *      counterpart), what PCA covariates, mixed models and a relatedness cut-off start from.  Parity with GCTA / PLINK is
 *      UNPINNED, as for "IBS": the expressions below are this project's definition.  The form is GCTA's per-pair-N estimator
 *      with the diagonal computed as every other element is (PLINK 1.9's default diagonal).
 *
 *      A GRM weights every variant by 1 / (2 p (1 - p)) INSIDE the sum, so no product of genotype planes gives it exactly.  The
 *      standardised genotypes are therefore quantised, BY DEFINITION, to 16-bit fixed point, and the matrix is an exact integer
 *      computation: it does not depend on tile order, row ranges, batches, streams or devices.
 *
 *      Genotype class g and validity of an HPGV8 byte are exactly those of "IBS"; n0, n1, n2 are a row's class counts over the
 *      columns below n_cols (hpgv_ibs_class_counts_dev).  Per row, with frac_bits s in [0, 14] and min_maf, f64 without
 *      contraction in this order:
 *          X = 2 n0 + n1      Y = n1 + 2 n2      T = X + Y      p = (double)Y / (double)T      d = sqrt(2.0 * p * (1.0 - p))
 *          z_c = ((double)c - 2.0 * p) / d   for c = 0, 1, 2      q_c = rint(z_c * 2^s), ties to even
 *      A row is USED iff it is not skipped, 0 < Y < T, (double)min(X, Y) / (double)T >= min_maf, and every |q_c| <= 32512
 *      (= 127 * 256).  An unused row's table is all zeros and the row takes no part, not even in n.  The limbs of q are
 *      lo = (int8)(q & 0xFF) and hi = (q - lo) / 256: q = 256 hi + lo exactly, hi in [-127, 127], lo in [-128, 127].  A missing
 *      byte has q = 0 and valid = 0.
 *
 *      Per pair i <= j, DIAGONAL INCLUDED, summed over the used rows where both columns are valid:
 *          sq = sum q_i q_j  (int64, exact)      n = sum 1      A_ij = ((double)sq * 2^(-2s)) / (double)n
 *      n = 0 gives the IEEE result (NaN).  On the matrix cores (csrc/hpgv_grm_kernels.h) sq = 65536 hi.hi + 256 (hi.lo + lo.hi)
 *      + lo.lo: five i8 products with exact i32 sums per range of at most 32 768 rows (|hi_i lo_j + lo_i hi_j| <= 32 512 per row),
 *      combined in int64.
 *
 *      Quantisation bound: |q_c 2^-s - z_c| <= delta = 2^-(s+1), so a pair's value lies within
 *      sum [delta (|z_i| + |z_j|) + delta^2] / n of the unquantised f64 sum of z_i z_j over n.  hpgv_grm_frac_bits(min_maf) is
 *      the largest s <= 14 with sqrt(2 (1 - min_maf) / min_maf) * 2^s <= 32512 -- no row at or above that MAF is lost to the
 *      |q_c| rule: 14 / 12 / 12 / 11 / 9 for min_maf 0.5 / 0.1 / 0.05 / 0.01 / 0.001, and -1 for min_maf outside (0, 0.5].
 *
 *      Out of scope: GCTA's Fhat3 diagonal, a text .grm.gz, a relatedness cut-off list, a 24-bit (three-limb) form, and a
 *      group form of the batch calls.  The principal components of the matrix: "PCA" below. */
typedef struct { int64_t sq, n; } hpgv_grm_acc;                                         /* 16 bytes */
/* d_class4: 4 int32 per row, {n0, n1, n2, missing} (hpgv_ibs_class_counts_dev).  d_skip, IN-OUT and required: a row that comes in
 * != 0 is unused whatever its counts; the call sets d_skip[row] = 1 for every unused row and leaves the others as they are.
 * d_tab: 8 bytes per row, {int8 hi[4], int8 lo[4]}, entries 0 .. 2 the classes and entry 3 zero; all zeros for an unused row:
 * every record written.  d_n_used (may be NULL): the call zeroes it on `stream` and counts the used rows into it.  One lane per
 * row; the table is bit for bit hpgv_grm_table's.  n_variants == 0 succeeds (and zeroes d_n_used).  HPGV_ERR_INVALID for
 * n_variants < 0, frac_bits outside [0, 14], min_maf outside [0, 0.5] or NaN, a NULL d_class4, d_skip or d_tab, d_class4 not
 * 16-byte, d_tab not 8-byte, d_n_used not 4-byte aligned.  Asynchronous on `stream`. */
int  hpgv_grm_table_dev(hpgv_ctx *ctx, const int32_t *d_class4, int n_variants, int frac_bits, double min_maf,
                        uint8_t *d_skip /* in-out, required */, uint8_t *d_tab, int32_t *d_n_used /* may be NULL */, void *stream);
/* Matrix, d_skip, alignment, refusals, streams and "profile" timing as hpgv_ibs_pairs_dev; d_tab and d_skip as
 * hpgv_grm_table_dev left them (with d_skip NULL every row takes part with its table: an unused row would then count in n).
 * The call ADDS {sq, n} of these rows to d_acc[i * n_cols + j] for 0 <= i <= j < n_cols with relaxed device-scope 64-bit
 * atomics and never touches an element with i > j; the caller zeroes the n_cols x n_cols records before the first call.
 * n_variants == 0 or n_cols < 1 succeed and write nothing.  d_tab must be 8-byte, d_acc 16-byte aligned.  A workgroup's row
 * range is never longer than 32 768 rows (hpgv_grm_plan_rows), so no i32 sum overflows whatever the shape. */
int  hpgv_grm_pairs_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols,
                        const uint8_t *d_skip, const uint8_t *d_tab, hpgv_grm_acc *d_acc /* n_cols x n_cols */, void *stream);

/* ---- PCA: the principal components of the GRM (GCTA's --pca, PLINK's --pca; no reference counterpart): the eigenpairs of
 *      largest magnitude of a symmetric f64 matrix that lies in device memory, by block subspace iteration with Rayleigh-Ritz.
 *      Parity with GCTA / PLINK is UNPINNED, as for "IBS" and "GRM": what follows is this project's definition.
 *
 *      With L = hpgv_pca_block(k) (16 for k <= 8, 32 for k <= 24) the solver keeps an n x L block Q with orthonormal columns:
 *        start    Q[i][c] = u - 0.5 with u the top 53 bits, as a fraction, of splitmix64's finaliser
 *                     x = seed + 0x9E3779B97F4A7C15 (32 i + c + 1);  x = (x ^ x >> 30) 0xBF58476D1CE4E5B9;
 *                     x = (x ^ x >> 27) 0x94D049BB133111EB;  x ^= x >> 31;  u = (x >> 11) 2^-53
 *                 (64-bit wrapping arithmetic: a function of (seed, row, column), not of a launch), then orthonormalised by
 *                 CholQR done twice: G = Q^T Q, G = R^T R (hpgv_pca_chol_inv), Q <- Q R^-1.
 *        sweep    Y = A Q (hpgv_pca_apply_dev);  H = Q^T Y, symmetrised (H + H^T) / 2 on the host;  H = W Theta W^T by
 *                 hpgv_pca_jacobi, the pairs by decreasing |theta|;  the residual block R = Y W - Q W Theta formed on the device and
 *                 its column norms taken (NOT w^T G w - theta^2, which cancels at about sqrt(eps));  converged when
 *                 max over i < k of ||r_i|| <= tol max|theta|;  otherwise Q <- Y orthonormalised as at the start.
 *        result   the k Ritz pairs of largest |theta|, written by DECREASING theta; vectors x = Q w of unit 2-norm, each with its
 *                 component of largest magnitude positive (the lowest index on a tie).
 *      Every sum over the n rows is taken in a fixed order (chunks of 256 rows, the partials added in chunk order; the block
 *      product's order is csrc/hpgv_pca_kernels.h's) and no floating-point atomic is used: the result depends on (A, n, k, tol,
 *      max_iter, seed) and nothing else -- not the device, its CU count, a stream or the run.
 *      The error of eigenvalue i falls by about lambda_{L+1} / lambda_i per sweep (in magnitudes).  A cohort with population
 *      structure has a few values well above the bulk and converges in some tens of sweeps; one WITHOUT structure, whose spectrum
 *      is one bulk, needs many.  Out of scope: Chebyshev or Krylov acceleration, a product that reads only the upper triangle of A
 *      (half the traffic, but a deterministic partial-sum scheme is needed), more than 24 pairs, a group form. */
/* The n_cols x n_cols records of hpgv_grm_pairs_dev as a full f64 matrix with row pitch lda (in elements; >= n_cols and even):
 * A[i][j] = A[j][i] = hpgv_grm_value of record [i][j] for i <= j, bit for bit.  Only records with i <= j are read.  A pair with
 * n = 0 gets 0.0 on both sides and is counted ONCE in *d_n_empty, which the call zeroes on `stream` first.  Elements with a
 * column index >= n_cols are not written.  n_cols == 0 succeeds.  HPGV_ERR_INVALID for frac_bits outside [0, 14], n_cols < 0,
 * lda < n_cols or odd, a NULL d_acc, d_A or d_n_empty, d_acc or d_A not 16-byte, d_n_empty not 8-byte aligned; HPGV_ERR_UNSUPPORTED
 * above 2 097 120 columns.  Asynchronous on `stream`. */
int  hpgv_grm_matrix_dev(hpgv_ctx *ctx, const hpgv_grm_acc *d_acc, int n_cols, int frac_bits,
                         double *d_A, size_t lda, uint64_t *d_n_empty, void *stream);
/* Y = A Q: A symmetric n x n f64, stored FULL with row pitch lda (elements; >= n and even; d_A 16-byte aligned), Q and Y n x L
 * row-major with pitch L, L = 16 or 32.  Elements of A at a row or column index >= n are never read; only the n x L elements of Y
 * are written.  Every element of Y is summed in ONE fixed order that depends on (n, L) only; no floating-point atomics: the
 * result is bit-identical from run to run.  A that is not symmetric gives A^T Q (a panel of rows is read as a panel of columns).
 * n == 0 succeeds.  HPGV_ERR_INVALID for another L, n < 0, lda < n or odd, a NULL pointer, a misaligned one.  Asynchronous on
 * `stream`; "profile" timing as hpgv_grm_pairs_dev. */
int  hpgv_pca_apply_dev(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, const double *d_Q, int L,
                        double *d_Y, void *stream);
/* The solver above on d_A (as hpgv_pca_apply_dev's; complete before the call).  Synchronous.  eigval[k], resid[k] = ||A x -
 * theta x|| as the last sweep measured it, vec[n x k] row-major, *n_iter the sweeps done, *converged 1 or 0 (all host memory).  At
 * max_iter without convergence the call still returns HPGV_OK with *converged = 0 and the last Ritz pairs with their true
 * residuals.  For n <= L the answer is hpgv_pca_jacobi of A copied to the host: *n_iter = 0, residuals computed on the host.
 * HPGV_ERR_INVALID for k < 1, k > 24, k > n, tol not positive or not finite, max_iter < 1, a NULL pointer, lda < n or odd, d_A not
 * 16-byte aligned.  HPGV_ERR_UNSUPPORTED when a Cholesky pivot fails: the matrix has RANK BELOW L (the block cannot keep L
 * independent columns), or is not finite. */
int  hpgv_pca_dev(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, int k, double tol, int max_iter, uint64_t seed,
                  double *eigval /* host, k */, double *vec /* host, n x k row-major */, double *resid /* host, k */,
                  int *n_iter, int *converged);

/* ---- Score: per-SAMPLE sums of per-variant weights times ALT counts (PLINK's --score; no reference counterpart): polygenic
 *      scores; with several weight columns the projection of a cohort onto principal-component loadings; with 0 / 1 weights a
 *      burden count per sample.  Parity with PLINK is UNPINNED, as for "IBS" and "GRM": what follows is this project's definition.
 *
 *      A score is one sum over every variant of a file -- across batches, engine threads and devices -- so, as the GRM is, it is
 *      quantised BY DEFINITION and summed as integers: 32-bit fixed-point weights in four i8 limbs on the matrix cores
 *      (csrc/hpgv_score_kernels.h).  The sums do not depend on tile order, row ranges, batches, streams or devices.
 *
 *      Genotype class g (0 / 1 / 2 ALT alleles), validity and pads of an HPGV8 byte are exactly those of "IBS"; n0, n1, n2 are a
 *      row's class counts over the columns below n_cols (hpgv_ibs_class_counts_dev).  Up to HPGV_SCORE_MAX = 32 scores per call
 *      (hpgv_pca_dev writes up to 24 components).
 *
 *      Inputs.  Per score k a frac_bits s_k in [-900, 900].  Per row the weights w[row * n_scores + k] (f64) and a flag byte:
 *      bit 0 = skip; bit 1 = flip, the weight names REF and the row contributes w (2 - g).  Per call one `impute` switch: != 0 is
 *      PLINK's default mean imputation, 0 its no-mean-imputation.
 *
 *      A row is USED iff it is not skipped, T = 2 (n0 + n1 + n2) > 0, every weight is finite, and every |q| <= 2^28 below.  An
 *      unused row takes no part in anything.  With p = (double)(n1 + 2 n2) / (double)T, per used row and score, f64 without
 *      contraction, rint to nearest with ties to even:
 *          q = rint(ldexp(w, s))
 *          not flipped:  qg = q    c = 0     qm = impute ? rint(ldexp(w * (2.0 * p), s))              : 0
 *          flipped:      qg = -q   c = 2 q   qm = impute ? rint(ldexp(w * (2.0 * (1.0 - p)), s)) - 2 q : -2 q
 *      A used row contributes c + qg g to column j on a called byte and c + qm on a missing one: a flipped called byte gives
 *      q (2 - g); a missing byte with imputation the imputed dosage times the weight; a missing byte without imputation exactly 0,
 *      flipped or not.  |qg|, |qm| and |c| are at most 2^30.  qg and qm are split into four BALANCED i8 limbs as the GRM splits q
 *      into two: l_0 = (int8)(v & 0xFF), v <- (v - l_0) / 256, and so on; v = l_0 + 256 l_1 + 65536 l_2 + 2^24 l_3 with the three
 *      low limbs in [-128, 127] and the top limb the rest (in [-64, 64]).
 *
 *      Accumulated, all int64 and exact:
 *          sum_k[j]    = sum over used rows of (qg_k g_j where j is called, qm_k where it is missing)
 *          const_k     = sum over used rows of c_k
 *          n_called[j] = used rows where j is called        n_alt[j] = sum over used rows of g_j        n_used = used rows
 *      Per sample:
 *          value_k[j] = ldexp((double)(sum_k[j] + const_k), -s_k)          (hpgv_score_value)
 *          avg_k[j]   = value_k[j] / (2.0 * (double)(impute ? n_used : n_called[j]))      (the IEEE result for 0)
 *
 *      Quantisation bound: |q 2^-s - w| <= 2^-(s+1), and likewise for the imputed term, so each used row moves a column's value
 *      by at most 2^-s (g <= 2) from the unquantised term w g (w (2 - g), w 2 p, w 2 (1 - p)).  hpgv_score_frac_bits(max_abs_w)
 *      returns 28 - e where frexp(max_abs_w) = m 2^e, 0.5 <= m < 1: |w| <= max_abs_w < 2^e gives |w 2^s| < 2^28, so no weight at or
 *      below max_abs_w trips the |q| rule (for max_abs_w below 2^928: above it the result is clamped to -900).
 *
 *      The table of a call's rows is LIMB-PLANE-MAJOR: int8 tab[(k * 8 + l) * tab_pitch + row], l = 0 .. 3 the limbs of qg_k and
 *      l = 4 .. 7 those of qm_k; tab_pitch a multiple of 64 and >= n_variants, zeros from n_variants to tab_pitch and for an
 *      unused row.  An operand of the matrix cores -- 16 rows of (score, limb) x 64 variants -- is then plain 16-byte loads.  Row 0
 *      of the table is row 0 of the matrix it is used with: a piece of a matrix has a table of its own.
 *
 *      Out of scope: dosage or probability input; multi-allelic records; PLINK's `center` and `variance-standardize` modifiers;
 *      computing SNP loadings from a PCA (a second pass shaped like the linear regression's product: the follow-up); a group form
 *      of the batch calls; more than 32 scores per call. */
#define HPGV_SCORE_MAX 32
#define HPGV_SCORE_SKIP 1                                                                /* flag bits of a row */
#define HPGV_SCORE_FLIP 2
/* d_class4 and d_skip (IN-OUT, required) as hpgv_grm_table_dev's: a row that comes in != 0 is unused, and the call sets
 * d_skip[row] = 1 for every unused row.  d_w: n_variants x n_scores doubles; d_flags: one byte per row; frac_bits: HOST array of
 * n_scores.  d_tab: 8 n_scores planes of tab_pitch bytes, every byte written (layout above).  d_const: int64[n_scores + 1]; the
 * call ADDS const_k of these rows to d_const[k] and their n_used to d_const[n_scores] with relaxed device-scope 64-bit atomics
 * (the caller zeroes it before the first call).  One lane per row; the table is bit for bit hpgv_score_table's.  tab_pitch == 0
 * succeeds.  HPGV_ERR_INVALID for n_variants < 0, n_scores outside 1 .. 32, a frac_bits outside [-900, 900], tab_pitch not a
 * multiple of 64 or < n_variants, a NULL pointer, d_class4 or d_tab not 16-byte, d_w or d_const not 8-byte aligned.  A non-finite
 * weight makes its row unused.  Asynchronous on `stream`. */
int  hpgv_score_table_dev(hpgv_ctx *ctx, const int32_t *d_class4, int n_variants, const double *d_w, const uint8_t *d_flags,
                          int n_scores, const int *frac_bits, int impute, uint8_t *d_skip /* in-out, required */,
                          int8_t *d_tab, size_t tab_pitch, int64_t *d_const, void *stream);
/* Matrix, d_skip, refusals, streams and "profile" timing as hpgv_ibs_pairs_dev; d_tab and d_skip as hpgv_score_table_dev left
 * them (with d_skip NULL every row takes part with its table: an unused row would then count in n_called and n_alt).  The call
 * ADDS sum_k[j] of these rows to d_acc[k * acc_pitch + j] for k < n_scores, n_called[j] to plane n_scores and n_alt[j] to plane
 * n_scores + 1, j < n_cols, with relaxed device-scope 64-bit integer atomics -- calls on pieces of a matrix, on several streams
 * and from several threads accumulate into one buffer -- and touches no other element; the caller zeroes the (n_scores + 2) x
 * acc_pitch int64 before the first call.  No floating-point atomics.  n_variants == 0 or n_cols < 1 succeed and write nothing.
 * HPGV_ERR_INVALID also for n_scores outside 1 .. 32, tab_pitch not a multiple of 64 or < n_variants, acc_pitch < n_cols, d_tab
 * not 16-byte or d_acc not 8-byte aligned.  A workgroup's row range is never longer than 2^22 rows (hpgv_score_plan_rows), so no
 * i32 sum overflows whatever the shape. */
int  hpgv_score_cols_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols,
                         const uint8_t *d_skip, const int8_t *d_tab, size_t tab_pitch, int n_scores,
                         int64_t *d_acc, size_t acc_pitch, void *stream);

/* ---- the variant-sharded resident scan of a GROUP context: what the runner's worker loop
 *      (assoc_runner.c:106-207, tdt_runner.c:150-200, stats_runner.c:176-215) becomes when the cohort lies in the HBM of
 *      the group's devices.  Variants are independent (assoc.c:38-82, tdt.c:41-271), so member g owns the contiguous
 *      shard [g*V/G, (g+1)*V/G) of the V variants (hpgv_group_shard), scans it on a stream of its own, and the ONE
 *      exchange is the gather of the per-variant results onto member 0: grouped ncclSend / ncclRecv over a communicator
 *      the group owns (ncclCommInitAll over the members' devices, RCCL over xGMI; librccl is loaded when
 *      hpgv_group_comm_init is called, not before).  Per-sample counters (get_sample_stats, stats_runner.c:197-198) are
 *      the one sum over variants: ncclReduce onto member 0.
 *      d_gt[g] / d_is_x[g]: member g's shard on ITS device, in the tool's engine layout (d_is_x or its entries may be
 *      NULL).  Result arrays: on member 0's device, sized for all V variants, variant v at index v (the *_dev entry
 *      points' element layouts).  The calls are asynchronous: they return when everything is queued; results are
 *      complete after hpgv_group_sync.  The gather of one call overlaps the scans of the next (each member keeps two
 *      generations of result scratch), so a caller that pipelines alternates between two sets of result arrays.
 *      A device may be listed twice only if it is member 0's (the one-GPU test rig): such members hand their results
 *      over by a device-local copy instead of RCCL, which refuses one device twice. ------------------------------ */
int  hpgv_group_comm_init(hpgv_ctx *group);               /* idempotent; HPGV_ERR_UNSUPPORTED without librccl */
int  hpgv_group_comm_ranks(const hpgv_ctx *group);        /* ranks of the group's communicator (ncclCommCount); 0 before init */
/* can librccl be loaded in this process ($HPGV_RCCL_LIB, then the usual names)?  HPGV_OK or HPGV_ERR_UNSUPPORTED;
 * `why` (may be NULL) receives the loader's messages for the candidates that failed.  Needs no context and no device. */
int  hpgv_group_rccl_probe(char *why, size_t why_cap);
int  hpgv_group_shard(const hpgv_ctx *group, int64_t n_variants, int member, int64_t *lo, int64_t *hi);
int  hpgv_group_assoc(hpgv_ctx *group, int task, const uint8_t *const *d_gt, const uint8_t *const *d_is_x,
                      int64_t n_variants, int32_t *d_counts /* V x 4 */, double *d_odds,
                      double *d_chisq /* NULL for Fisher */, double *d_p);
int  hpgv_group_tdt(hpgv_ctx *group, const uint8_t *const *d_gt, const uint8_t *const *d_is_x, int64_t n_variants,
                    int32_t *d_tu /* V x 2 */, double *d_odds, double *d_chisq, double *d_p);
/* d_sample_missing (n_samples ints on member 0, may be NULL) is OVERWRITTEN with the sum over every member's shard */
int  hpgv_group_stats(hpgv_ctx *group, const uint8_t *const *d_gt, int64_t n_variants, int32_t *d_counts8 /* V x 8 */,
                      double *d_hwe_chi2, double *d_hwe_p, int32_t *d_sample_missing);
int  hpgv_group_sync(hpgv_ctx *group);
/* The epistasis scan over the group's devices (the reference deals block coordinates to its workers,
 * singlenode/epistasis_runner.c:114-145).  hpgv_epi_set_dataset / hpgv_epi_set_folds / hpgv_epi_set_fold_masks on a GROUP
 * context give every member the dataset and the folds.  A combination belongs to its first SNP; hpgv_group_epi_share tells
 * which first SNPs [i_begin, i_end) member `member` takes -- runs with (nearly) equal numbers of combinations, for pairs cut
 * at multiples of 64.  hpgv_group_epi_rank: every member ranks its share on its own device (order 2 and 3: the tile scans;
 * 4 and 5: the listed-combination kernel), the members' per-fold top lists are gathered onto member 0 over the group's
 * communicator and merged: outputs as hpgv_epi_rank_order (8 mask words per model; orders 2 and 3 use the first),
 * identical to the one-device ranking.  Synchronous.  *scan_ms (may be NULL): the slowest member's scan time. */
int  hpgv_group_epi_share(const hpgv_ctx *group, int order, int member, int *i_begin, int *i_end);
int  hpgv_group_epi_rank(hpgv_ctx *group, int order, int subset, int max_ranking_size, int32_t *combs_out,
                         double *accuracy, uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms);

/* duration (ms) of the last scan / statistics kernel launched through this ctx
 * when option "profile" = 1 (HIP events on the launch stream; synchronises) */
int  hpgv_last_kernel_ms(hpgv_ctx *ctx, float *scan_ms, float *stats_ms);

/* ---- per-batch host entry points (synchronous; what assoc_test / tdt_test /
 *      get_variants_stats adapters call).  gt: host, variant-major, VCF column
 *      order, rows `pitch` bytes apart.  Outputs: caller-allocated arrays of
 *      n_variants elements; chisq may be NULL for Fisher.  Thread-safe: may be
 *      called concurrently from the runner's worker threads. ---------------- */
int  hpgv_assoc(hpgv_ctx *ctx, int task, const uint8_t *gt, size_t pitch, int n_variants,
                const uint8_t *is_x,
                int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                double *odds, double *chisq, double *p);
/* hpgv_assoc with task CHISQ plus the label permutation's two outputs ("label permutation" above): n_ge (n_variants
 * int32) and batch_max (n_perms doubles of the labels set with hpgv_set_perm_labels, overwritten).  Synchronous and
 * thread-safe; a group context deals it to its members as hpgv_assoc.  HPGV_ERR_STATE without labels. */
int  hpgv_assoc_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                     int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                     double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max);
/* The model tests ("model tests" above) of a host batch in VCF column order: counts8 (n_variants x 8 int32), chisq5 and p5
 * (n_variants x 5 doubles, [v * 5 + HPGV_MODEL_*]) through the assoc layout, the class scan and the statistics kernel.  n_ge and
 * batch_max both NULL: no permutation, and no labels are needed; both non-NULL: the trend permutation's outputs as
 * hpgv_assoc_perm's (HPGV_ERR_STATE without labels); exactly one of them NULL: HPGV_ERR_INVALID.  Synchronous and thread-safe; a
 * group context deals it to its members as hpgv_assoc. */
int  hpgv_assoc_model(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants,
                      int32_t *counts8, double *chisq5, double *p5, int32_t *n_ge, double *batch_max);
int  hpgv_tdt(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants,
              const uint8_t *is_x, int32_t *t1, int32_t *t2,
              double *odds, double *chisq, double *p);
/* hpgv_tdt plus the family flips' two outputs ("family flips" above): n_ge (n_variants int32) and batch_max (n_perms doubles of
 * the flips set with hpgv_set_tdt_flips, overwritten).  Synchronous and thread-safe; a group context deals it to its members as
 * hpgv_tdt.  HPGV_ERR_STATE without flips. */
int  hpgv_tdt_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants,
                   const uint8_t *is_x, int32_t *t1, int32_t *t2,
                   double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max);
int  hpgv_stats(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants,
                int32_t *counts8 /* n_variants x 8 */, double *hwe_chi2, double *hwe_p);
/* same batch, additionally: sample_missing (n_samples ints, ACCUMULATED into; may be NULL) and, for
 * every variant whose four biallelic cells do not cover all called genotypes, its 256-bin genotype
 * table: multi_idx[k] = variant index, multi_table[k*256 + code]; *n_multi in = capacity of both
 * arrays (in variants), out = number of such variants (filled up to the capacity). */
int  hpgv_stats_ex(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants,
                   int32_t *counts8, double *hwe_chi2, double *hwe_p, int32_t *sample_missing,
                   int32_t *multi_idx, int32_t *multi_table, int *n_multi);

/* the stats counters per phenotype group of hpgv_set_stats_groups (one report per phenotype,
 * stats_runner.c:300-303,319-323): counts8[(g * n_variants + v) * 8 + k], hwe_*[g * n_variants + v]
 * (both hwe arrays may be NULL).  Samples in no group are not counted anywhere. */
int  hpgv_stats_groups(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants,
                       int32_t *counts8, double *hwe_chi2, double *hwe_p);

/* epistasis dataset rows of vcf2epi (epistasis_dataset_process_records, dataset_creator.c:241-272):
 * out[v * (n_affected + n_unaffected) + destination] with cases first then controls, each in VCF column
 * order (group_individuals_by_phenotype, :302-320), codes 0 "0/0", 1 heterozygous, 2 homozygous
 * non-reference, 255 missing.  Uses the cohort of hpgv_set_cohort. */
int  hpgv_epi_dataset(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, uint8_t *out);

/* hpgv_stats_ex (+ hpgv_mendel) on a batch of VCF text: what get_variants_stats and get_sample_stats need
 * (stats_runner.c:194-198, aggregate_runner.c:113-114), tokenized on the device.  sample_missing (n_samples ints)
 * and child_errors (one per trio of hpgv_set_pedigree) are ACCUMULATED into; mendel_errors[v] per line; any of the
 * three may be NULL.  Multi-allelic lines as in hpgv_stats_ex. */
int  hpgv_stats_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                     uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *counts8,
                     double *hwe_chi2, double *hwe_p, int32_t *sample_missing, int32_t *multi_idx,
                     int32_t *multi_table, int *n_multi, int32_t *mendel_errors, int32_t *child_errors);

/* the same with the counters of every phenotype group of hpgv_set_stats_groups in addition (one report per phenotype,
 * stats_runner.c:300-303,319-323): group_counts8[(g * max_lines + v) * 8 + k], group_hwe_*[g * max_lines + v]; all three
 * may be NULL (then this is hpgv_stats_text) */
int  hpgv_stats_text_groups(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                            uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *counts8,
                            double *hwe_chi2, double *hwe_p, int32_t *sample_missing, int32_t *multi_idx,
                            int32_t *multi_table, int *n_multi, int32_t *mendel_errors, int32_t *child_errors,
                            int32_t *group_counts8, double *group_hwe_chi2, double *group_hwe_p);

/* record filters of the text entry points, computed on the device from the tokenized matrix before the tool's own
 * scan: --maf (keep minor-allele frequency >= min_maf), --missing (keep missing-genotype rate <= max_missing),
 * --mendel (keep Mendelian errors <= max_mendel_errors) -- shared_options.c:44-46,101-115; the filter bodies live
 * in hpg-libs (definitions as hpgv_stats_filter_dev / hpgv_mendel_scan_dev).  A negative value switches a filter off.
 * A rejected line gets HPGV_LINE_FILTERED OR-ed into its status; its statistics are still computed.  The count
 * filters need hpgv_set_stats_cohort(n_samples), the Mendel filter hpgv_set_pedigree over the same columns. */
#define HPGV_LINE_FILTERED 0x100
int  hpgv_set_text_filters(hpgv_ctx *ctx, double min_maf, double max_missing, long max_mendel_errors);
/* the inheritance filters of the same text entry points: --inh-dom (min_dominant) and --inh-rec (min_recessive),
 * shared_options.c:42-56.  The filter bodies live in hpg-libs; the definitions here, on the counts c0 .. c5 of
 * hpgv_inheritance_scan_dev:
 *   dominant followers  = c1 + c4          (affected carriers, unaffected 0/0)
 *   recessive followers = c2 + (c3 - c5)   (affected homozygous non-reference, unaffected not so)
 *   fraction            = followers / (c0 + c3), computed in double
 * A record is kept when every active fraction >= its threshold; a record with no counted call fails.  A negative value
 * switches that filter off; a value above 1 is HPGV_ERR_INVALID.  A group context applies it to every member.  A batch
 * with an inheritance filter set lays the raw matrix out as HPGV_LAYOUT_ASSOC and scans it: it needs hpgv_set_cohort
 * over the same columns (else HPGV_ERR_STATE). */
int  hpgv_set_text_inheritance_filters(hpgv_ctx *ctx, double min_dominant, double min_recessive);

/* hpg-var-vcf filter (filter_runner.c:23-260): the record filters alone.  hpgv_filter_text tokenizes a batch of VCF text
 * as the other *_text calls do (line_off, field_off, status as there; the text on the device when hpgv_text_alias says so),
 * applies the device filters of hpgv_set_text_filters and hpgv_set_text_inheritance_filters (HPGV_LINE_FILTERED in status)
 * and runs no tool's scan.  The count
 * filters read the layout of hpgv_set_stats_cohort, which this call needs whatever the filters.  The call keeps the device
 * text it tokenized, and that text's line starts, for hpgv_text_partition on the same `text`: until that call, or the next
 * hpgv_filter_text on `text`, one of the context's stream slots stays with it.  When *n_lines > max_lines nothing is kept. */
int  hpgv_filter_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                      uint64_t *line_off, uint32_t *field_off, int32_t *status);
/* The lines the last hpgv_filter_text on `text` tokenized, partitioned on the device that holds them (the uploaded copy,
 * or the aliased window on its member's device): keep[i] != 0 lines first, in line order, then the others in line order,
 * copied into `out` (out_cap bytes; page-locked memory is copied at the bus rate).  *total_bytes = the bytes of the lines
 * (line_off[n_lines] - line_off[0] on the device), *kept_bytes = those of the kept lines; both may be NULL.  n_lines must
 * be what hpgv_filter_text returned.  keep = NULL only releases the hold.  Synchronous. */
int  hpgv_text_partition(hpgv_ctx *ctx, const char *text, const uint8_t *keep, int n_lines, char *out, size_t out_cap,
                         uint64_t *kept_bytes, uint64_t *total_bytes);
/* The device primitive: lines i = 0 .. n_lines - 1 of d_text, line i = bytes [d_line_off[i], d_line_off[i + 1]), into d_out:
 * every line with d_keep[i] != 0, byte for byte and back to back in line order, then every other line in line order.  d_out
 * receives exactly d_line_off[n_lines] - d_line_off[0] bytes and nothing outside them is stored; d_text and d_out may have
 * any alignment.  *d_kept_bytes (device memory, may be NULL) = the bytes of the kept lines.  d_scratch:
 * hpgv_lines_partition_scratch_bytes(n_lines) bytes of device memory (8-byte aligned).  Asynchronous on `stream`. */
size_t hpgv_lines_partition_scratch_bytes(int n_lines);
int  hpgv_lines_partition_dev(hpgv_ctx *ctx, const char *d_text, const uint64_t *d_line_off, int n_lines, const uint8_t *d_keep,
                              char *d_out, uint64_t *d_kept_bytes, void *d_scratch, void *stream);
/* hpg-var-vcf split (split_runner.c:23-190): the same partition with n_buckets ways.  Lines [first_line, first_line +
 * n_lines) of the text the last hpgv_filter_text on `text` holds, line first_line + k going to bucket bucket[k]: every line
 * of bucket 0 back to back in line order, then those of bucket 1, ..., copied into `out`.  bucket_off (host, n_buckets + 1
 * entries): bucket b occupies out[bucket_off[b] .. bucket_off[b + 1]), bucket_off[n_buckets] = the bytes stored, which must
 * fit in out_cap.  A line whose id is >= n_buckets goes nowhere.  n_buckets: 1 .. 256.  Unlike hpgv_text_partition this
 * releases nothing: call it for as many line ranges as needed, then hpgv_text_partition(..., keep = NULL, ...).  The
 * uploaded copy, an aliased window and group contexts as there.  Synchronous. */
int  hpgv_text_multisplit(hpgv_ctx *ctx, const char *text, const uint8_t *bucket, int first_line, int n_lines, int n_buckets,
                          char *out, size_t out_cap, uint64_t *bucket_off);
/* The device primitive: lines i = 0 .. n_lines - 1 of d_text (as for hpgv_lines_partition_dev) into d_out, the lines of
 * bucket b = d_bucket[i] back to back in line order from d_bucket_off[b], the buckets one after another in id order,
 * d_bucket_off[n_buckets] = the end (device memory, n_buckets + 1 entries).  A line with d_bucket[i] >= n_buckets is not
 * stored; nothing outside [d_out, d_out + d_bucket_off[n_buckets]) is stored; d_text and d_out may have any alignment.
 * n_buckets = 2 with d_bucket = !keep gives hpgv_lines_partition_dev's bytes.  n_buckets: 1 .. 256, and n_buckets x
 * ceil(n_lines / 64) below INT_MAX.  d_scratch: hpgv_lines_multisplit_scratch_bytes(n_lines, n_buckets) bytes of device
 * memory (8-byte aligned).  Asynchronous on `stream`. */
size_t hpgv_lines_multisplit_scratch_bytes(int n_lines, int n_buckets);
int  hpgv_lines_multisplit_dev(hpgv_ctx *ctx, const char *d_text, const uint64_t *d_line_off, int n_lines, const uint8_t *d_bucket,
                               int n_buckets, char *d_out, uint64_t *d_bucket_off, void *d_scratch, void *stream);
/* The same for rows of one length: the rows i of d_src (src_pitch apart) with d_keep[i] != 0 go to consecutive rows of d_dst
 * (dst_pitch apart) in source order, row_bytes of each.  d_index (n_rows int32): the destination row of row i, or -1;
 * *d_n_kept: the number of kept rows (0 for n_rows == 0).  Three launches for flags -> exclusive scan (the partition's scan, over
 * ones) and one copy kernel, which moves whole 16-byte granules where both pitches and both pointers are multiples of 16 and
 * single bytes otherwise.  Nothing is stored outside the kept rows' row_bytes: the bytes between two destination rows and behind
 * the last one keep what they held.  The caller sizes d_dst for the rows it keeps (n_rows of them at most).  d_scratch:
 * hpgv_rows_gather_scratch_bytes(n_rows) bytes of device memory, 8-byte aligned.  HPGV_ERR_INVALID for n_rows < 0, a pitch below
 * row_bytes, a NULL d_n_kept, and with n_rows > 0 a NULL d_keep, d_index or d_scratch (d_src and d_dst may be NULL only with
 * row_bytes == 0).  Asynchronous on `stream`. */
size_t hpgv_rows_gather_scratch_bytes(int n_rows);
int  hpgv_rows_gather_dev(hpgv_ctx *ctx, const uint8_t *d_src, size_t src_pitch, size_t row_bytes, int n_rows,
                          const uint8_t *d_keep, uint8_t *d_dst, size_t dst_pitch, int32_t *d_index /* n_rows: destination row or -1 */,
                          int32_t *d_n_kept, void *d_scratch, void *stream);

/* BGZF written on the device: what the filter and split runners write with HPGV_OUT_BGZF.
 * The device primitive: d_text in n_segs segments, segment s = bytes [d_seg_off[s], d_seg_off[s + 1]) (device memory,
 * n_segs + 1 entries).  Every segment is cut into blocks of at most HPGV_BGZF_BLOCK_TEXT bytes and every block becomes a
 * complete BGZF member: the 18-byte header bgzip writes (MTIME 0, XFL 0, OS 255, the BC subfield with BSIZE), a raw DEFLATE
 * payload in one final block (fixed Huffman codes; stored when that would be no smaller than the text, so that a member
 * never exceeds 65 536 bytes), CRC-32 and ISIZE.  The members lie back to back in d_out in segment order;
 * d_seg_out_off (device memory, n_segs + 1 entries): segment s's members are d_out[d_seg_out_off[s] .. d_seg_out_off[s + 1]),
 * an empty segment has none.  No EOF block is written: the caller ends a file with the 28-byte constant.  The same text and
 * segments give the same bytes on every run.  Nothing outside [d_out, d_out + d_seg_out_off[n_segs]) is stored; d_text and
 * d_out may have any alignment.  d_out holds hpgv_bgzf_deflate_bound(text_bytes, n_segs) bytes and d_scratch
 * hpgv_bgzf_deflate_scratch_bytes(text_bytes, n_segs) bytes of device memory (16-byte aligned), text_bytes being no less
 * than d_seg_off[n_segs] - d_seg_off[0].  Asynchronous on `stream`. */
#define HPGV_BGZF_BLOCK_TEXT 65280
size_t hpgv_bgzf_deflate_bound(uint64_t text_bytes, int n_segs);
size_t hpgv_bgzf_deflate_scratch_bytes(uint64_t text_bytes, int n_segs);
int  hpgv_bgzf_deflate_dev(hpgv_ctx *ctx, const char *d_text, const uint64_t *d_seg_off, int n_segs, uint8_t *d_out,
                           uint64_t *d_seg_out_off, void *d_scratch, void *stream);
/* The same on host buffers: `text` as one segment, its members into `out`, *out_bytes = their bytes.  When they exceed
 * out_cap the call returns HPGV_ERR_INVALID and leaves `out` untouched: hpgv_bgzf_deflate_bound(text_bytes, 1) always
 * fits.  Synchronous; thread-safe like the other host-buffer calls. */
int  hpgv_bgzf_compress(hpgv_ctx *ctx, const char *text, size_t text_bytes, uint8_t *out, size_t out_cap, size_t *out_bytes);
/* hpgv_text_partition with its two parts deflated on the device before they are copied back: `out` receives the kept
 * lines' members, then -- unless want_rest is 0: the other lines are then neither deflated nor copied -- the other lines'
 * members.  comp_bytes[2] = the bytes of the two runs of members; kept_bytes / total_bytes are the text's, as there.
 * last_byte[2] = the last text byte of either part ('\n' for an empty one): what a writer needs to end a file's last
 * line.  comp_bytes and last_byte may be NULL.  Holds, group contexts and aliased windows as hpgv_text_partition; members
 * beyond out_cap: HPGV_ERR_INVALID, `out` untouched (hpgv_bgzf_deflate_bound(total_bytes, 2) always fits). */
int  hpgv_text_partition_bgzf(hpgv_ctx *ctx, const char *text, const uint8_t *keep, int n_lines, uint8_t *out, size_t out_cap,
                              int want_rest, uint64_t *kept_bytes, uint64_t *total_bytes, uint64_t *comp_bytes, uint8_t *last_byte);
/* hpgv_text_multisplit with every bucket deflated: bucket b's members are out[bucket_off[b] .. bucket_off[b + 1]), a
 * bucket without lines has none.  last_byte (n_buckets entries, may be NULL) as above.  Releases nothing, as the plain
 * call; hpgv_bgzf_deflate_bound(bytes of the lines, n_buckets) always fits. */
int  hpgv_text_multisplit_bgzf(hpgv_ctx *ctx, const char *text, const uint8_t *bucket, int first_line, int n_lines, int n_buckets,
                               uint8_t *out, size_t out_cap, uint64_t *bucket_off, uint8_t *last_byte);

/* the same rows from a batch of VCF text (tokenized on the device like hpgv_assoc_text): row v of `out` belongs to
 * line v; lines that are not records (field_off[10 v + 5] == 0xFFFFFFFF) leave their row undefined */
int  hpgv_epi_dataset_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                           uint64_t *line_off, uint32_t *field_off, int32_t *status, uint8_t *out);

/* ---- epistasis / MDR counting (hpg-var-gwas epi: src/gwas/epistasis/model.c, mdr.c, epistasis.c;
 *      runner src/gwas/epistasis/singlenode/epistasis_runner.c) -------------------------------------
 * The input is the vcf2epi dataset (dataset.c:63-76; hpgv_epi_dataset makes its rows): one row per SNP,
 * n_affected + n_unaffected bytes, cases first, 0 / 1 / 2 = genotype, anything else = missing.  The cell
 * of a combination of `order` SNPs is numbered with the LAST SNP varying fastest
 * (get_genotype_combinations, dataset.c:170-200): order 2 -> cell = g_i * 3 + g_j. */
enum { HPGV_EPI_TESTING = 0, HPGV_EPI_TRAINING = 1 };                 /* enum evaluation_subset, model.h:73 */

/* Wide limits.  Without option "epi_wide" the packed kernels' limits hold: at most 16 folds, fewer than 65 536 samples per
 * (fold, class) group (every scan), at most 65 535 samples per class (triples, listed combinations, orders 4 and 5); what is
 * past them is refused with HPGV_ERR_UNSUPPORTED.  With "epi_wide" >= 1:
 *   - hpgv_epi_set_folds / _set_fold_masks take 1 .. 64 folds and groups of any size; hpgv_epi_set_dataset gives a class of
 *     65 536 or more the implicit single fold too.  A layout with more than 16 folds or a group of 65 536 or more is WIDE-ONLY;
 *   - hpgv_epi_eval_combs, hpgv_epi_rank_order[_rows], hpgv_epi_counts[_all_folds]: the wide kernel when the layout is wide-only
 *     or a class exceeds 65 535;
 *   - hpgv_epi_rank_triples[_rows]: in the same cases the any-order ranking at order 3 (same outputs; no "no empty fold" rule);
 *   - hpgv_epi_rank_pairs[_rows]: the any-order ranking at order 2 for a wide-only layout; a class of 65 536 or more in
 *     smaller groups keeps k_epi_pairs;
 *   - hpgv_group_epi_rank: the same, member by member.
 * Still refused, with or without the option:
 *   - hpgv_epi_scan_pairs / hpgv_epi_scan_triples on a wide-only layout (the dense scans read the staging tables such a layout
 *     does not have: use hpgv_epi_eval_combs), and hpgv_epi_scan_triples with a class above 65 535;
 *   - more than 64 folds (the fold tables of the wide kernel's launches);
 *   - order > 5 (the 64-byte model record holds 243 cells);
 *   - genotype planes of 2^32 words or more (V x 3 x padded samples / 32: the kernels address them with 32-bit word offsets). */
/* copies the dataset to the device; until folds are given all samples form one fold (none when a class holds 65536 samples
 * or more and "epi_wide" is 0: such a cohort needs hpgv_epi_set_folds before any scan) */
int  hpgv_epi_set_dataset(hpgv_ctx *ctx, const uint8_t *genotypes, int n_variants, int n_affected, int n_unaffected);
/* k-fold cross-validation: fold_of_sample[s] in [0, num_folds) = the fold whose TESTING part holds sample s
 * (get_k_folds, cross_validation.c:16-100); num_folds <= 16, fewer than 65536 samples per class and fold ("epi_wide": 64 folds,
 * any group size) */
int  hpgv_epi_set_folds(hpgv_ctx *ctx, const int32_t *fold_of_sample, int num_folds);
/* the same from the reference's own mask array (get_k_folds_masks, cross_validation.c:247-281):
 * num_folds x num_samples_with_padding bytes, 1 = training part, both classes padded to 16.  Masks that
 * are not a partition (a sample left out of no fold, or of two) are refused with HPGV_ERR_UNSUPPORTED. */
int  hpgv_epi_set_fold_masks(hpgv_ctx *ctx, const uint8_t *fold_masks, int num_folds);
/* combination_counts (model.c:76-124) of listed combinations (order 2 to 5, 3^order cells; combs = n_combs x order
 * SNP indices): counts_*[comb * cells + cell].  Orders 4 and 5: at most 65535 samples per class ("epi_wide": any) */
int  hpgv_epi_counts(hpgv_ctx *ctx, int order, const int32_t *combs, int n_combs,
                     int32_t *counts_aff, int32_t *counts_unaff);
/* combination_counts_all_folds (model.c:126-206), the reference's layout for n_combs combinations in a
 * row: counts_*[(fold * n_combs + comb) * cells + cell] = count over the TRAINING part of the fold */
int  hpgv_epi_counts_all_folds(hpgv_ctx *ctx, int order, const int32_t *combs, int n_combs,
                               int32_t *counts_aff, int32_t *counts_unaff);
/* process_set_of_combinations (epistasis.c:14-95) for every pair (i, j), i_begin <= i < i_end, i < j:
 * per fold the MDR high-risk cells (mdr_high_risk_combinations2 on the training counts), the confusion
 * matrix on `subset` and the balanced accuracy (test_model, model.c:320-335).  Outputs, pairs in
 * lexicographic order: accuracy[fold * *n_pairs + p], risky_mask[...] (bit c = cell c is high risk).
 * Call with accuracy = risky_mask = NULL to get *n_pairs only.  Refuses a wide-only layout ("Wide limits"). */
int  hpgv_epi_scan_pairs(hpgv_ctx *ctx, int i_begin, int i_end, int subset, double *accuracy,
                         uint16_t *risky_mask, unsigned long long *n_pairs);
/* the whole scan with the per-fold ranking of the runner (add_to_model_ranking, model.c:478-517; ties:
 * higher accuracy, then smaller (i, j)): for every fold the best max_ranking_size pairs,
 * out[fold * max_ranking_size + k], n_ranked[fold] of them.  *scan_ms (may be NULL) = device time of
 * the scan kernels.  A wide-only layout ("epi_wide") is ranked by the any-order ranking at order 2. */
int  hpgv_epi_rank_pairs(hpgv_ctx *ctx, int subset, int max_ranking_size, int32_t *comb_i, int32_t *comb_j,
                         double *accuracy, uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms);
/* the same over the pairs (i, j) with i_begin <= i < i_end only (i_begin a multiple of 64): the unit of work of
 * one GPU when the triangle is cut into row bands; the bands' lists merge into the whole ranking */
int  hpgv_epi_rank_pairs_rows(hpgv_ctx *ctx, int i_begin, int i_end, int subset, int max_ranking_size,
                              int32_t *comb_i, int32_t *comb_j, double *accuracy, uint32_t *risky_mask,
                              int32_t *n_ranked, float *scan_ms);

/* order 3: the same model for every triple i < j < k (27 cells, cell = (g_i * 3 + g_j) * 3 + g_k; at most 65535
 * samples per class, no empty fold).  hpgv_epi_scan_triples is the dense form for small sets (<= 256 SNPs):
 * accuracy / risky_mask[((fold * V + i) * V + j) * V + k], NaN / 0 where (i, j, k) is no triple;
 * hpgv_epi_rank_triples the per-fold ranking as for pairs.  With "epi_wide" hpgv_epi_rank_triples[_rows] take classes above
 * 65535 and wide-only layouts (the any-order ranking at order 3); hpgv_epi_scan_triples refuses both. */
int  hpgv_epi_scan_triples(hpgv_ctx *ctx, int subset, double *accuracy, uint32_t *risky_mask);
int  hpgv_epi_rank_triples(hpgv_ctx *ctx, int subset, int max_ranking_size, int32_t *comb_i, int32_t *comb_j,
                           int32_t *comb_k, double *accuracy, uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms);
/* ... over the triples whose FIRST SNP lies in [i_begin, i_end) only (one device's share, as hpgv_epi_rank_pairs_rows) */
int  hpgv_epi_rank_triples_rows(hpgv_ctx *ctx, int i_begin, int i_end, int subset, int max_ranking_size, int32_t *comb_i,
                                int32_t *comb_j, int32_t *comb_k, double *accuracy, uint32_t *risky_mask, int32_t *n_ranked,
                                float *scan_ms);

/* ANY order the reference's --order takes (main_epistasis.c:128,142), here 2 <= order <= 5 (3^order cells, cell = the
 * genotypes of the SNPs as base-3 digits, the last SNP the lowest: get_genotype_combinations, dataset.c:170-200; at most
 * 65535 samples per class; "epi_wide": any class and group size, up to 64 folds, on k_epi_combs_wide).  The pair and triple scans above are the fast forms of orders 2 and 3; these take the
 * combinations as a LIST and work one lane per cell.
 * hpgv_epi_eval_combs: process_set_of_combinations (epistasis.c:14-95) of n_combs listed combinations (n_combs x order SNP
 * indices): accuracy[comb * num_folds + fold], risky_mask[(comb * num_folds + fold) * 8 + w] (bit c % 32 of word c / 32 =
 * cell c is high risk; may be NULL).
 * hpgv_epi_rank_order: every combination i0 < i1 < ... of the dataset, per fold the best max_ranking_size (the runner's
 * add_to_model_ranking, model.c:478-517; ties: higher accuracy, then the smaller combination):
 * combs_out[(fold * max_ranking_size + k) * order + s], accuracy[fold * max_ranking_size + k],
 * risky_mask[(fold * max_ranking_size + k) * 8 + w], n_ranked[fold].  _rows: only the combinations whose FIRST SNP lies in
 * [i_begin, i_end) -- one device's share when the first SNPs are dealt out; the shares' lists merge into the whole ranking. */
int  hpgv_epi_eval_combs(hpgv_ctx *ctx, int order, const int32_t *combs, int n_combs, int subset, double *accuracy,
                         uint32_t *risky_mask);
int  hpgv_epi_rank_order(hpgv_ctx *ctx, int order, int subset, int max_ranking_size, int32_t *combs_out, double *accuracy,
                         uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms);
int  hpgv_epi_rank_order_rows(hpgv_ctx *ctx, int order, int i_begin, int i_end, int subset, int max_ranking_size,
                              int32_t *combs_out, double *accuracy, uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms);

/* what the last hpgv_epi_rank_pairs[_rows] / _triples[_rows] / _order[_rows] call of this context ran: the scan kernel its
 * launches used (as the dispatch chose it: the options ask for a kernel, the dataset's shape can rule it out), the number of
 * scan launches, and how many of them had to be repeated because a fold's candidate list overflowed.
 * kernel = HPGV_EPI_KERNEL_NONE when the call launched nothing. */
enum {
    HPGV_EPI_KERNEL_NONE = 0,
    HPGV_EPI_KERNEL_PAIRS_MFMA = 1,      /* k_epi_pairs_mfma: pair cell counts on the matrix cores */
    HPGV_EPI_KERNEL_PAIRS_VALU = 2,      /* k_epi_pairs: pair cell counts on the vector ALU */
    HPGV_EPI_KERNEL_TRIPLES_MFMA = 3,    /* k_epi_triples_mfma */
    HPGV_EPI_KERNEL_TRIPLES3 = 4,        /* k_epi_triples3: the 27 cells nine at a time */
    HPGV_EPI_KERNEL_TRIPLES1 = 5,        /* k_epi_triples1 (ablation builds only) */
    HPGV_EPI_KERNEL_TRIPLES = 6,         /* k_epi_triples: two passes */
    HPGV_EPI_KERNEL_COMBS = 7,           /* k_epi_combs: listed combinations of any order */
    HPGV_EPI_KERNEL_COMBS_WIDE = 8       /* k_epi_combs_wide: the same with 32-bit counts and up to 64 folds (option "epi_wide") */
};
typedef struct hpgv_epi_rank_info {
    int32_t kernel;                      /* HPGV_EPI_KERNEL_* */
    int32_t launches;                    /* scan launches, relaunches included */
    int32_t relaunches;                  /* launches whose candidate list overflowed: their rows were scanned again, fewer at a time */
    int32_t reserved;
} hpgv_epi_rank_info;
int  hpgv_epi_last_rank_info(hpgv_ctx *ctx, hpgv_epi_rank_info *info);

/* Mendelian errors of a host batch: errors[v] per variant (may be NULL) and child_errors[t] per trio of
 * hpgv_set_pedigree, ACCUMULATED into (may be NULL) */
int  hpgv_mendel(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                 int32_t *errors, int32_t *child_errors);

/* ---- bgzip-compressed VCF text (--compression bgzip, shared_options.c:60-61): the raw-DEFLATE payloads of BGZF blocks
 * decoded on the device, one wave per block (any number of blocks per call; option inflate_wave = 0: one lane per block,
 * which wants a hundred thousand blocks per call).  Block b occupies d_comp[in_off[b] .. + in_len[b]) and decodes to exactly
 * out_len[b] <= 65 536 bytes at d_text + out_off[b]; d_status[b] is 0, or non-zero for a block this decoder does not take (the
 * caller decodes it on the host).  d_comp must be readable for 8 bytes past the end of the last block, d_text for 8 bytes
 * past the last block's text.  Asynchronous on `stream`. */
/* "the text of the batch is on the device at d_text already" (e.g. decoded there by hpgv_inflate_blocks_dev): a *_text entry
 * point called with host_text then tokenizes d_text in place, copies nothing up, and WRITES INTO host_text (a buffer of at
 * least text_bytes bytes) the heads of the lines -- each line up to its first sample column, CHROM .. FORMAT, or the whole
 * line when it has fewer than ten fields -- back to back; line_off[i] is the offset of line i's head in host_text, field_off
 * stays relative to the line start.  d_text = NULL removes the entry. */
int  hpgv_text_alias(hpgv_ctx *ctx, const char *host_text, const char *d_text);
/* ... and d_text is a WINDOW of a text the bgzip decoder left on the device together with the tokenizer's tile records
 * (hpgv_bgzf_verify_tiles_dev): d_text_base = where that text begins (d_text lies text-bytes inside it and begins a line),
 * d_tiles its records, n_tiles how many of them are valid.  The *_text entry points then tokenize the window WITHOUT their
 * counting sweep over it -- the text is read once (the window's last tile is counted again up to the window's end; a window
 * that reaches beyond the valid records is tokenized the ordinary way).  Same results, bit for bit. */
int  hpgv_text_alias_tiles(hpgv_ctx *ctx, const char *host_text, const char *d_text, const char *d_text_base,
                           const void *d_tiles, uint64_t n_tiles);
int  hpgv_inflate_blocks_dev(hpgv_ctx *ctx, const uint8_t *d_comp, const uint64_t *d_in_off, const uint32_t *d_in_len,
                             const uint64_t *d_out_off, const uint32_t *d_out_len, int n_blocks, uint8_t *d_text,
                             int32_t *d_status, void *stream);
/* The CRC-32 check of decoded BGZF blocks (what htslib's bgzf reader / zlib's gzread do per block behind --compression bgzip,
 * shared_options.c:60-61): for every block with d_status 0, the CRC-32 of its text against the block's trailer, which follows
 * its payload (the four bytes at d_comp + in_off + in_len); a mismatch sets d_status to HPGV_BLOCK_BAD_CRC.  Same tables as
 * hpgv_inflate_blocks_dev; asynchronous on `stream`. */
#define HPGV_BLOCK_BAD_CRC 9
int  hpgv_bgzf_verify_dev(hpgv_ctx *ctx, const uint8_t *d_comp, const uint64_t *d_in_off, const uint32_t *d_in_len,
                          const uint64_t *d_out_off, const uint32_t *d_out_len, int n_blocks, const uint8_t *d_text,
                          int32_t *d_status, void *stream);
/* The same check, and -- the wave that has just read a block's text being the cheapest place to do it -- the VCF tokenizer's
 * records of that text: per 2 KiB tile of the decoded text (tile k = bytes [2048 k, 2048 k + 2048) from d_text on) its newline
 * count, the TABs behind its last newline and where that newline is, which is all the tokenizer's first sweep computes.
 * d_tiles: hpgv_text_tiles_bytes(text bytes) bytes of device memory, ZEROED before the first call for a text; n_tiles: how
 * many records it may write (blocks whose text lies beyond are only checked).  Blocks the decoder refused (d_status != 0
 * on entry) and blocks that leave with HPGV_BLOCK_BAD_CRC mark every tile they touch "count again": their text is the
 * caller's to patch, and no record counted from the text that was there is used for it.  See hpgv_text_alias_tiles. */
size_t hpgv_text_tiles_bytes(uint64_t text_bytes);
int  hpgv_bgzf_verify_tiles_dev(hpgv_ctx *ctx, const uint8_t *d_comp, const uint64_t *d_in_off, const uint32_t *d_in_len,
                                const uint64_t *d_out_off, const uint32_t *d_out_len, int n_blocks, const uint8_t *d_text,
                                int32_t *d_status, void *d_tiles, uint64_t n_tiles, void *stream);
/* The rows of those tables from the compressed bytes of a bgzip file on the device (bgzf.c of htslib writes the blocks the
 * reference reads with --compression bgzip, shared_options.c:60-61): the blocks that form a chain from byte `lo` (a block
 * start; 0 at first) and end at or before `hi` (bytes [0, hi) are on the device), at most max_rows of them, written from
 * index 0 on; out_off counts from text_base.  result[0] = rows, [1] = where the chain stands (the next call's lo),
 * [2] = text_base + the text bytes of the rows, [3] = block headers seen in [lo, hi).  No rows although a whole block lies
 * in the range: the file's headers are not the ones bgzip writes, and the caller walks it itself.  Returns when `result`
 * is filled.  d_scratch: hpgv_bgzf_scan_scratch_bytes(hi - lo, max_rows) bytes of device memory. */
size_t hpgv_bgzf_scan_scratch_bytes(uint64_t range_bytes, int max_rows);
int  hpgv_bgzf_scan_dev(hpgv_ctx *ctx, const uint8_t *d_comp, uint64_t lo, uint64_t hi, uint64_t text_base, int max_rows,
                        uint64_t *d_in_off, uint32_t *d_in_len, uint64_t *d_out_off, uint32_t *d_out_len,
                        void *d_scratch, size_t scratch_bytes, uint64_t *result, void *stream);

/* ---- VCF text -> HPGV8 on the GPU (replaces the per-genotype
 *      strdup + get_alleles of assoc.c:45-56 / tdt.c:97-108,150-157) ------------------
 * text: whole VCF DATA lines (no '#' header lines), TAB separated, '\n' terminated (the last
 * line may lack it), CHROM..FORMAT then n_samples sample columns.  Outputs, all optional
 * except gt:  line_off[max_lines+1] byte offset of each line start (line_off[n_lines] = end);
 * field_off[line*10 + k] offset, relative to the line start, of field k = CHROM..FORMAT (0..8)
 * and of the first sample column (9) so the host can build result records without re-scanning;
 * gt rows in VCF column order (strict != 0: genotypes get_alleles() would not report as
 * ALLELES_OK become 0xFF; a NUL byte inside a sample column ends that column's string, as it does in the
 * reference's char* samples); is_x per line (assoc.c:94 rule); status per line: 0 ok, 1 fewer
 * than 10 columns, 2 FORMAT has no GT (row all missing), 3 fewer sample columns than n_samples.
 * More than max_lines lines: the first max_lines are parsed and *n_lines reports the true count.
 * *n_lines = -1 (hpgv_tokenize_dev only, after the stream has been waited for): the one-sweep form (option tokenizer_tiles = 2)
 * gave up waiting for another workgroup's record -- set the option to 1 and call again; hpgv_tokenize and the *_text
 * entry points do that themselves. */
int  hpgv_tokenize_dev(hpgv_ctx *ctx, const char *d_text, size_t text_bytes, int n_samples, int strict,
                       int max_lines, int *d_n_lines, uint64_t *d_line_off, uint32_t *d_field_off,
                       uint8_t *d_gt, size_t pitch, uint8_t *d_is_x, int32_t *d_status, void *stream);
/* host buffers in and out (synchronous) */
int  hpgv_tokenize(hpgv_ctx *ctx, const char *text, size_t text_bytes, int n_samples, int strict,
                   int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off,
                   uint8_t *gt, size_t pitch, uint8_t *is_x, int32_t *status);

/* text batch in, statistics out: tokenize + layout + scan + statistics without the genotype
 * matrix ever crossing PCIe.  task as hpgv_assoc; outputs sized max_lines; *n_lines = lines in
 * the text (results are filled for min(*n_lines, max_lines)); line_off / field_off / status as
 * hpgv_tokenize (may be NULL).  The cohort (hpgv_set_cohort / hpgv_set_families) fixes n_samples. */
int  hpgv_assoc_text(hpgv_ctx *ctx, int task, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                     uint64_t *line_off, uint32_t *field_off, int32_t *status,
                     int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                     double *odds, double *chisq, double *p);
/* hpgv_assoc_text -- every argument up to p unchanged, the same outputs bit for bit -- which then, in the same slot and on
 * the same stream, SELECTS lines: a small kernel builds one flag per line from the p-values on the device and the statuses,
 * and line i is selected iff it is a record (status byte 0), is not HPGV_LINE_FILTERED, and p[i] <= p_max.  A NaN p is never
 * selected; p == p_max is.  sel (sized max_lines): the number of the line among this call's selected lines, in line order, or
 * -1.  The selected lines' genotype rows -- VCF column order, n_samples bytes each, from the call's raw matrix, the form
 * hpgv_ld and hpgv_ld_edges take -- are compacted on the device (hpgv_rows_gather_dev's kernels) and only that block is
 * copied out: row k of rows_out (rows_pitch >= n_samples bytes apart) is the line with sel == k.  *n_sel is the number of
 * selected lines; where it exceeds rows_cap no row is copied and sel is still valid (call again with room, or gather from a
 * copy of the rows).  rows_out may be NULL when rows_cap is 0.  status may be NULL (the record filters then do not run, as in
 * hpgv_assoc_text).  A NaN p_max, a NULL sel or n_sel, rows_cap < 0 and rows_pitch < n_samples are HPGV_ERR_INVALID.  On a
 * GROUP context the call is dealt to a member exactly as hpgv_assoc_text is: batches are independent. */
int  hpgv_assoc_select_text(hpgv_ctx *ctx, int task, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                            uint64_t *line_off, uint32_t *field_off, int32_t *status,
                            int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                            double *odds, double *chisq, double *p,
                            double p_max, int32_t *sel, uint8_t *rows_out, size_t rows_pitch, int rows_cap, int *n_sel);
/* hpgv_assoc_text with task CHISQ plus n_ge (sized max_lines) and batch_max (n_perms doubles, overwritten): tokenizer,
 * HPGV_LAYOUT_ASSOC layout, scan, chi-square, then the permutation kernel.  The lines a caller of hpgv_assoc_text drops --
 * status 1 (not a record) and lines a record filter rejected (HPGV_LINE_FILTERED) -- take no part in batch_max and get
 * n_ge = 0. */
int  hpgv_assoc_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                          uint64_t *line_off, uint32_t *field_off, int32_t *status,
                          int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                          double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max);
/* hpgv_assoc_model on a text: tokenizer, HPGV_LAYOUT_ASSOC layout, class scan, statistics and -- with n_ge (sized max_lines)
 * and batch_max (n_perms doubles, overwritten) both non-NULL -- the trend form of the permutation kernel; counts8 sized
 * max_lines x 8, chisq5 and p5 max_lines x 5.  n_ge / batch_max as in hpgv_assoc_model.  Lines that are not records (status
 * 1) or that a record filter rejected (HPGV_LINE_FILTERED) take no part in the permutation, exactly as in
 * hpgv_assoc_perm_text.  The text path runs the kernel chain; it has no one-pass form. */
int  hpgv_assoc_model_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                           uint64_t *line_off, uint32_t *field_off, int32_t *status,
                           int32_t *counts8, double *chisq5, double *p5, int32_t *n_ge, double *batch_max);
int  hpgv_tdt_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                   uint64_t *line_off, uint32_t *field_off, int32_t *status,
                   int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p);
/* hpgv_tdt_text plus n_ge (sized max_lines) and batch_max (n_perms doubles, overwritten): tokenizer, HPGV_LAYOUT_TDT layout, scan,
 * statistics, then the flip kernels.  Lines that are not records (status 1) or that a record filter rejected
 * (HPGV_LINE_FILTERED) take no part in batch_max and get n_ge = 0, as in hpgv_assoc_perm_text. */
int  hpgv_tdt_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                        uint64_t *line_off, uint32_t *field_off, int32_t *status,
                        int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max);

/* ---- LD on a host batch and on a text ("LD" above; synchronous, thread-safe) ------------------------------------------- */
/* gt: n_variants rows in VCF column order, `pitch` bytes apart (pitch >= n_samples).  The rows go through the
 * HPGV_LAYOUT_ASSOC layout and then hpgv_ld_window_dev with b_begin = 0: the LD is over the cohort columns (AFFECTED and
 * UNAFFECTED).  chrom / pos (host, per row): both or both NULL (else HPGV_ERR_INVALID); max_bp < 0 = no distance limit.
 * r2: n_variants x window doubles; counts6 (may be NULL) x 6 int32.  HPGV_ERR_STATE without hpgv_set_cohort; window outside
 * 1 .. HPGV_LD_MAX_WINDOW is HPGV_ERR_UNSUPPORTED.  A GROUP context returns HPGV_ERR_UNSUPPORTED: dealing batches to the
 * members would cut the band at every seam. */
int  hpgv_ld(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int window, const int32_t *chrom /* may be NULL */,
             const uint32_t *pos /* may be NULL */, int64_t max_bp, double *r2, int32_t *counts6 /* may be NULL */);
/* The edge form on a host batch: rows, layout, state and refusals as hpgv_ld (a GROUP context: HPGV_ERR_UNSUPPORTED), then
 * hpgv_ld_edges_dev with b_begin = 0; a NaN min_r2 is HPGV_ERR_INVALID.  On return *n_edges is the true number of pairs with
 * r2 >= min_r2.  Where it is <= edge_cap, edges[0 .. *n_edges) holds them sorted by (b, a) (sorted on the host after the copy);
 * where it is larger the content of `edges` is unspecified and the caller calls again with room.  edges may be NULL when
 * edge_cap is 0. */
int  hpgv_ld_edges(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int window, const int32_t *chrom /* may be NULL */,
                   const uint32_t *pos /* may be NULL */, int64_t max_bp, double min_r2, hpgv_ld_edge *edges, uint64_t edge_cap,
                   uint64_t *n_edges);
/* tokenizer -> assoc layout -> hpgv_ld_window_dev with no matrix crossing the bus, as hpgv_assoc_model_text.  EVERY line of the
 * text is one row of the window: a line with status 1 (not a record) or flagged HPGV_LINE_FILTERED is a skipped row -- it keeps
 * its slot, and its pairs are NaN with zero counts.  No distance filter here: line_off / field_off come back for the caller,
 * who knows the positions only then.  r2: max_lines x window doubles, min(*n_lines, max_lines) x window of them written;
 * counts6 (may be NULL) x 6.  status may be NULL.  State and refusals as hpgv_ld, a GROUP context included. */
int  hpgv_ld_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                  uint64_t *line_off, uint32_t *field_off, int32_t *status, int window, double *r2, int32_t *counts6 /* may be NULL */);

/* ---- IBS on a host batch and on a text ("IBS" above; synchronous, thread-safe) ------------------------------------------ */
/* gt: n_variants rows in VCF column order, `pitch` bytes apart (pitch >= n_samples).  The columns are those of the
 * HPGV_LAYOUT_STATS layout -- every sample, in VCF order; its bytes are stats flags, so the kernels read the HPGV8 rows
 * themselves, in the stats layout's pitch -- for hpgv_ibs_class_counts_dev and hpgv_ibs_pairs_dev with n_cols = n_samples.
 * skip (host, per row, may be NULL): != 0 = the row takes no part.  class4 (host): 4 int32 per row, zeros for a skipped row.
 * d_counts: DEVICE memory, n_samples x n_samples records, 16-byte aligned, zeroed by the caller before the first batch and
 * ACCUMULATED into; calls from several threads may share it.  HPGV_ERR_STATE without hpgv_set_stats_cohort.  A GROUP context
 * returns HPGV_ERR_UNSUPPORTED: the counts of a run lie on one device (a caller with several devices keeps one buffer per
 * device and adds them: integers, any order). */
int  hpgv_ibs(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *skip /* may be NULL */,
              int32_t *class4, hpgv_ibs_counts *d_counts);
/* tokenizer -> stats layout -> the same two kernels with no matrix crossing the bus.  A line with status 1 (not a record) or
 * flagged HPGV_LINE_FILTERED -- the lines a caller of hpgv_assoc_text drops -- is a skipped row, and so is a line the tokenizer
 * flags as chromosome X (CHROM exactly "X"; Y and MT get no rule, as elsewhere).  class4: max_lines x 4 int32,
 * *n_lines x 4 of them written, zeros for a skipped line.  Where *n_lines comes back larger than max_lines NOTHING was added to
 * d_counts and class4 is not written: the counts accumulate, so the caller calls again with room and no line is counted twice.
 * status may be NULL.  State and refusals as hpgv_ibs. */
int  hpgv_ibs_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                   uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *class4, hpgv_ibs_counts *d_counts);

/* ---- GRM on a host batch and on a text ("GRM" above; synchronous, thread-safe) ------------------------------------------ */
/* hpgv_ibs with the GRM's kernels: matrix, skip, class4 (zeros for a skipped row; a row that is unused for another reason keeps
 * its counts -- hpgv_grm_table of them tells), state and refusals as hpgv_ibs, plus HPGV_ERR_INVALID for frac_bits outside
 * [0, 14] or min_maf outside [0, 0.5].  Class counts, table and pair sums run on one stream; d_acc: DEVICE memory,
 * n_samples x n_samples records, 16-byte aligned, zeroed by the caller before the first batch and ACCUMULATED into, the
 * diagonal included.  A GROUP context returns HPGV_ERR_UNSUPPORTED. */
int  hpgv_grm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *skip /* may be NULL */,
              int frac_bits, double min_maf, int32_t *class4, hpgv_grm_acc *d_acc);
/* hpgv_ibs_text with the GRM's kernels: dropped lines and chromosome-X lines are skipped rows, and where *n_lines comes back
 * larger than max_lines NOTHING was added to d_acc and class4 is not written. */
int  hpgv_grm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                   uint64_t *line_off, uint32_t *field_off, int32_t *status, int frac_bits, double min_maf,
                   int32_t *class4, hpgv_grm_acc *d_acc);

/* ---- Score on a host batch and on a text ("Score" above; synchronous, thread-safe) -------------------------------------- */
/* hpgv_grm with the score's kernels: matrix, class4 (zeros for a skipped row), state and refusals as hpgv_ibs.  w: n_variants x
 * n_scores doubles, flags: one byte per row (HPGV_SCORE_SKIP, HPGV_SCORE_FLIP), frac_bits: n_scores ints, all host memory.
 * d_acc: DEVICE memory, (n_scores + 2) x acc_pitch int64 (hpgv_score_cols_dev), d_const: DEVICE memory, int64[n_scores + 1]
 * (hpgv_score_table_dev); both zeroed by the caller before the first batch and ACCUMULATED into; calls from several threads may
 * share them.  HPGV_ERR_INVALID -- before anything is launched -- for a weight that is not finite, n_scores outside 1 .. 32, a
 * frac_bits outside [-900, 900], acc_pitch < n_samples, d_acc or d_const NULL or not 8-byte aligned.  A GROUP context returns
 * HPGV_ERR_UNSUPPORTED (a caller with several devices keeps one pair of buffers per device and adds them: integers, any order). */
int  hpgv_score(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const double *w, const uint8_t *flags,
                int n_scores, const int *frac_bits, int impute, int32_t *class4, int64_t *d_acc, size_t acc_pitch, int64_t *d_const);
/* The first CALLBACK of this ABI.  The weights of a text's rows depend on the ID and allele fields of its lines, which only the
 * tokenizer finds: the line heads must come back to the host before the weights can be known, and the matrix the tokenizer wrote
 * must not cross the bus in between.  So hpgv_score_text, after tokenisation and before the score kernels, invokes `weigh` ONCE, on
 * the calling thread, with the text, the n_lines line_off / field_off / status entries of hpgv_assoc_text (they lie on the host
 * even where the caller passed NULL for them), and w (n_lines x n_scores) and flags (n_lines), both zeroed, to fill.  A non-zero
 * return ends the call with HPGV_ERR_INVALID and nothing added.  The callback runs while the call holds one of the context's slots:
 * it reads what it is given and fills w and flags, and makes no call on the same context. */
typedef int (*hpgv_score_weigh_fn)(void *user, const char *text, int n_lines, const uint64_t *line_off,
                                   const uint32_t *field_off, const int32_t *status, double *w, uint8_t *flags);
/* hpgv_grm_text with the score's kernels: dropped lines (status 1, HPGV_LINE_FILTERED) and chromosome-X lines are skipped rows
 * WHATEVER the callback says, and where *n_lines comes back larger than max_lines NOTHING was added, class4 is not written and
 * `weigh` was not invoked.  A non-finite weight from the callback is HPGV_ERR_INVALID with nothing added.  Otherwise as hpgv_score. */
int  hpgv_score_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                     uint64_t *line_off, uint32_t *field_off, int32_t *status, hpgv_score_weigh_fn weigh, void *user,
                     int n_scores, const int *frac_bits, int impute, int32_t *class4,
                     int64_t *d_acc, size_t acc_pitch, int64_t *d_const);

/* ---- label permutation, host side: no GPU call, no context, usable without a device ------------------------------- */
/* n_perms label rows for hpgv_set_perm_labels, labels_out[p * n_samples + j]: row p is a uniform shuffle of the cohort
 * columns' conditions (1 = affected), so every row has as many ones as the cohort has affected samples; HPGV_COND_OTHER
 * columns get 0.  Deterministic in (seed, p): the generator is counter-based, SplitMix64 (Steele, Lea and Flood 2014;
 * mix(z): z += 0x9E3779B97F4A7C15, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB,
 * z ^ z >> 31): row p's key is mix(seed ^ mix(p)), its draw number i is mix(key + i), i = 0, 1, ...  Fisher-Yates over the
 * cohort columns in VCF order, from the last position down: position k - 1 swaps with position (draw * k) >> 64, k = n .. 2. */
int  hpgv_perm_labels_shuffle(const uint8_t *condition, int n_samples, int n_perms, uint64_t seed, uint8_t *labels_out);
/* The same within strata, for hpgv_assoc_cmh_perm*: stratum_of_sample as hpgv_set_strata takes it (any non-negative value is a
 * stratum here; what a HPGV_COND_OTHER column holds is not read).  Row p has hpgv_perm_labels_shuffle's key and draws; the strata
 * are walked in ascending order of their number and each runs the same Fisher-Yates walk over ITS cohort columns in VCF order, the
 * draw counter running on from one stratum to the next.  So every stratum keeps its number of affected samples in every row, and
 * row p does not depend on n_perms.  A cohort column with a negative stratum keeps its observed label; HPGV_COND_OTHER columns
 * get 0.  HPGV_ERR_INVALID for a negative count or a NULL pointer it needs. */
int  hpgv_perm_labels_shuffle_within(const uint8_t *condition, const int32_t *stratum_of_sample, int n_samples, int n_perms,
                                     uint64_t seed, uint8_t *labels_out);
/* n_perms flip rows for hpgv_set_tdt_flips, flips_out[p * n_families + f]: every family of every row flipped with probability
 * 1/2, independently.  Deterministic in (seed, p, f), from the same counter-based generator and row keys as the label rows: row
 * p's key is mix(seed ^ mix(p)), and family f's flip is bit f & 63 of mix(key + (f >> 6)) -- one 64-bit word per 64 families. */
int  hpgv_perm_flips_shuffle(int n_families, int n_perms, uint64_t seed, uint8_t *flips_out);
/* With P = n_perms permutations, t_max the element-wise maximum of every batch's batch_max (in any order; it is sorted here
 * and each variant's rank found by binary search):
 *     emp1[v] = (n_ge[v] + 1) / (P + 1)                           pointwise
 *     emp2[v] = (#{p : t_max[p] >= t_obs[v]} + 1) / (P + 1)       family-wise, max(T)
 * both NaN where t_obs[v] is NaN.  n_perms < 1: HPGV_ERR_INVALID. */
int  hpgv_perm_pvalues(const double *t_obs, int n_variants, const int32_t *n_ge, const double *t_max, int n_perms,
                       double *emp1, double *emp2);
/* r2 of six counts {n, sa, sb, saa, sbb, sab} by the expression of "LD" above: the function the kernel's epilogue calls, built for
 * the host.  No GPU call, no context. */
double hpgv_ld_r2(const int32_t counts6[6]);
/* Clump assignment (PLINK's default --clump, without overlap and without replication) of n candidates with p-values p and the
 * undirected LD edges between them (hpgv_ld_edges' records; a and b are candidate numbers, duplicates are harmless, r2 is not
 * read: the threshold was applied when the list was made).  Candidates are visited by ascending p, ties by ascending number; a
 * NaN p is skipped; the visit stops at the first p > p1 (p == p1 is visited).  A visited candidate that is already claimed is
 * skipped.  Otherwise it becomes the index of a new clump -- index_of[i] = i, and i is appended to clump_order -- and claims
 * every not yet claimed candidate j joined to it by an edge: index_of[j] = i.  Everything else gets index_of = -1.
 * clump_order (n entries of room, may be NULL) holds *n_clumps entries on return.  An endpoint outside 0 .. n - 1 is
 * HPGV_ERR_INVALID, and so are n < 0 and a NULL p, index_of or n_clumps.  O(n log n + n_edges).  No GPU call, no context. */
int  hpgv_clump(int n, const double *p, const hpgv_ld_edge *edges, uint64_t n_edges, double p1,
                int32_t *index_of, int32_t *clump_order /* may be NULL */, int *n_clumps);
/* The five terms {t00, t01, t02, t11, t12} of one row's class counts by the expressions of "IBS" above; returns 1 for a used row
 * (T >= 4), else 0 with zeros (a negative count included).  Whether the row is skipped is the caller's to know.  No GPU call. */
int  hpgv_ibs_terms(int32_t n0, int32_t n1, int32_t n2, double t[5]);
/* out = {Z0, Z1, Z2, PI_HAT, DST} of one pair's counts with E = {E00, E01, E02, E11, E12}: the function k_ibs_select calls,
 * built for the host.  No GPU call, no context. */
void hpgv_ibs_genome(const hpgv_ibs_counts *c, const double E[5], double out[5]);
/* rows per row range of hpgv_ibs_pairs_dev's launch on a device with n_cus compute units: a multiple of 64, never above 2^31 - 64 */
int  hpgv_ibs_plan_rows(int n_variants, int n_cols, int n_cus);
/* One row's table by the expressions of "GRM" above: hi[c], lo[c] for the classes c = 0, 1, 2, entry 3 zero; returns 1 for a
 * used row, else 0 with zeros (a negative count or a frac_bits outside [0, 14] included).  Whether the row is skipped is the
 * caller's to know.  The function k_grm_table calls, built for the host.  No GPU call. */
int  hpgv_grm_table(int32_t n0, int32_t n1, int32_t n2, int frac_bits, double min_maf, int8_t hi[4], int8_t lo[4]);
/* the largest frac_bits at which no row with MAF >= min_maf is lost ("GRM" above); -1 for min_maf outside (0, 0.5] */
int  hpgv_grm_frac_bits(double min_maf);
/* A_ij of one record: ((double)sq * 2^(-2 frac_bits)) / (double)n */
double hpgv_grm_value(const hpgv_grm_acc *a, int frac_bits);
/* rows per row range of hpgv_grm_pairs_dev's launch on a device with n_cus compute units: a multiple of 64, never above 32 768 */
int  hpgv_grm_plan_rows(int n_variants, int n_cols, int n_cus);
/* One row's table by the expressions of "Score" above: limbs[k * 8 + l], l = 0 .. 3 the limbs of qg_k and 4 .. 7 those of qm_k,
 * and c[k], for k < n_scores; returns 1 for a used row, else 0 with zeros (a negative count, n_scores outside 1 .. 32 or a
 * frac_bits outside [-900, 900] included; nothing is written for a NULL pointer or a bad n_scores).  flags: HPGV_SCORE_SKIP,
 * HPGV_SCORE_FLIP.  The function k_score_table calls, built for the host.  No GPU call. */
int  hpgv_score_table(int32_t n0, int32_t n1, int32_t n2, const double *w, int n_scores, const int *frac_bits, int flags,
                      int impute, int8_t *limbs /* n_scores x 8 */, int64_t *c /* n_scores */);
/* 28 - e with frexp(max_abs_w) = m 2^e, clamped to [-900, 900]: the largest frac_bits at which no weight with |w| <= max_abs_w
 * makes its row unused ("Score" above, with the argument; it holds for max_abs_w < 2^928).  0 for 0; INT_MIN for a NaN, an
 * infinity or a negative number. */
int  hpgv_score_frac_bits(double max_abs_w);
/* value of one sum: ldexp((double)(sum + cnst), -frac_bits) */
double hpgv_score_value(int64_t sum, int64_t cnst, int frac_bits);
/* rows per row range of hpgv_score_cols_dev's launch on a device with n_cus compute units: a multiple of 64, never above 2^22 */
int  hpgv_score_plan_rows(int n_variants, int n_cols, int n_scores, int n_cus);
/* The host pieces of "PCA" above.  No GPU call. */
/* the block width of a k-pair solve: 16 for 1 <= k <= 8, 32 for k <= 24, -1 otherwise */
int  hpgv_pca_block(int k);
/* Cyclic Jacobi eigen-decomposition of the symmetric L x L matrix H (row-major, L <= 32; (H + H^T) / 2 is what is solved): on
 * return column j of H is the unit eigenvector of theta[j], the pairs by decreasing |theta| (the lower diagonal position first
 * among equals).  HPGV_ERR_INVALID for L outside [1, 32] or a NULL pointer. */
int  hpgv_pca_jacobi(int L, double *H, double *theta);
/* G = R^T R by Cholesky (R upper triangular) and M = R^-1, L x L row-major, L <= 32.  Returns 0, or 1 when a pivot fell to or
 * below L * DBL_EPSILON * (the largest diagonal element of G) or is NaN: G is singular to working precision or indefinite, and
 * M is then not to be used.  -1 for L outside [1, 32] or a NULL pointer. */
int  hpgv_pca_chol_inv(int L, const double *G, double *M);

/* streaming-read ceiling probe: reads `bytes` from d_buf with the scan's load
 * shape and no arithmetic; returns the kernel time in ms (diagnostic) */
int  hpgv_read_probe(hpgv_ctx *ctx, const uint8_t *d_buf, size_t bytes, int iters, float *ms);
/* f64 matrix-core ceiling probe: 8 workgroups of four waves per CU, every wave `steps` rounds of eight independent
 * v_mfma_f64_16x16x4_f64 and no memory traffic; *ms: the kernel time (mean of iters launches after one), *flop: the floating-point
 * operations of one launch, 2 x 16 x 16 x 4 per instruction (diagnostic: what tools/bench_linear_perm.py holds the permutation
 * kernel against) */
int  hpgv_mfma_f64_probe(hpgv_ctx *ctx, int steps, int iters, float *ms, double *flop);

#ifdef __cplusplus
}
#endif
#endif
