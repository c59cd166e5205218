/*
 * hpgv_host_internal.h -- what the translation units of libhpgv_host.so share: the engine binding and its caches
 * (host_engine.c), the thread teams (host_pool.c), the byte sources and readers of the file runners (host_source.c,
 * host_inflate.c, host_bgzf.c, host_reader.c), the result formatting (host_format.c, host_output.c).  Nothing here is part
 * of the library's interface (include/hpgv_host.h is): every symbol below has hidden visibility.
 *
 *   host_containers.c  the hpg-libs stand-in containers and records (array_list, list_t, result structs)
 *   host_stage.c       sample strings -> one byte per genotype (hpgv_host_stage_records)
 *   host_engine.c      the process-wide engine context, page-locked / device buffer caches, shutdown
 *   host_adapters.c    assoc_test, tdt_test, get_variants_stats, get_sample_stats
 *   host_output.c      the reference's writers (assoc_runner.c:292-342, tdt_runner.c:286-304) and the in-process sort
 *   host_epistasis.c   k-folds, the epistasis run and its report
 *   host_pool.c        sleeping thread teams, NUMA placement
 *   host_source.c      PED table, byte sources (plain / gzip / bgzip)
 *   host_inflate.c     raw DEFLATE on the host
 *   host_bgzf.c        bgzip files staged and decoded on the device(s)
 *   host_reader.c      whole-line batches, the VCF header
 *   host_format.c      result lines of a batch, the writer thread
 *   host_vcftools.c    the VCF tools' batch steps and writers: filter partition, split keys and files
 *   host_records.c     the record filters of hpgv_run_set_record_filters: regions, coverage, variant types, inheritance
 *   host_sideout.c     what a run keeps beside its result file and writes at its end: .mperm, .clumped, the stats report
 *   host_covar.c       the covariate file of the logistic and linear runs (and the latter's phenotype file): read whole, matched to the VCF's sample names; the within file of the CMH run by the same reader
 *   host_pca.c         the principal components of a run's relationship matrix, or of .grm.bin files: .eigenval, .eigenvec
 *   host_runner.c      the file runners' pipeline and their runs (hpgv_run_*)
 */
#ifndef HPGV_HOST_INTERNAL_H
#define HPGV_HOST_INTERNAL_H
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include "hpgv_host.h"
#include <fcntl.h>
#include <math.h>
#include <sched.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#pragma GCC visibility push(hidden)

extern hpgv_ctx *g_ctx;

/* The bgzip device path may run in PARTS, one per member of a group context (bgzf_parts_stage): the threads that stage,
 * decode and hand out a part work on that member's device.  They say so once -- ctx_use(member context, member index) --
 * and everything below them that allocates, copies or launches uses CTX, and the per-member caches (streams, the decoded
 * text) slot t_member.  Threads that never say so work on g_ctx, which for a group is its first member: the single-device
 * path is unchanged. */
enum { MEMBERS_MAX = 16 };
extern __thread hpgv_ctx *t_ctx;
extern __thread int t_member;
#define CTX (t_ctx ? t_ctx : g_ctx)
typedef struct { hpgv_ctx *ctx; int member; } ctx_saved_t;
static inline ctx_saved_t ctx_use(hpgv_ctx *ctx, int member) { ctx_saved_t o = { t_ctx, t_member }; t_ctx = ctx; t_member = ctx ? member : 0; return o; }
static inline void ctx_back(ctx_saved_t o) { t_ctx = o.ctx; t_member = o.member; }

typedef void (*pool_fn)(void *arg, int task);
typedef struct {
    pthread_t *th; int n_threads;
    pthread_mutex_t mu; pthread_cond_t cv_work, cv_done;
    pool_fn fn; void *arg; int n_tasks, next, running, gen, stop;
} io_pool_t;

enum { DEV_TEXT_FIXED = 0, DEV_TEXT_GROWS = 1 };

typedef struct { list_item_t *first, *last; size_t n; } item_chain_t;
static inline void chain_add(item_chain_t *c, list_item_t *it) {
    if (!it) return;
    it->next_p = NULL;
    if (c->last) c->last->next_p = it; else c->first = it;
    c->last = it; c->n++;
}

typedef struct {
    int n;
    char **fid, **iid, **pat, **mat, **phe;             /* phe: the PHENO column as written (the stats tool's variable) */
    int *sex, *pheno;
    char *blob;
} ped_table_t;

enum { SRC_RAW = 0, SRC_BGZF = 1, SRC_GZIP = 2 };
/* a BGZF block table, a row per block: its payload's place in the file, its text's place in the decoded text */
typedef struct { uint64_t *in_off, *out_off; uint32_t *in_len, *out_len; size_t n, cap; } bgzf_rows_t;

typedef struct {
    int kind, fd;
    off_t pos, size;                                    /* RAW: next unread byte, file size */
    const unsigned char *map; size_t map_pos;           /* BGZF: the mapped compressed file, next block */
    unsigned char *pend; size_t pend_len, pend_pos;     /* BGZF: a block inflated aside because the caller's room was short */
    size_t *blk;                                        /* BGZF: per-call block table (offset, length, destination, size) */
    io_pool_t *pool;                                    /* team for the pread segments / the block inflation (may be NULL) */
    char *job_buf; size_t job_want; int job_bad;        /* the job the team is working on */
    gzFile gz;                                          /* GZIP */
    /* BGZF decoded on the GPU: the whole file's text in device memory, handed out window by window */
    void *d_comp, *d_text, *rstream, *cstream; size_t dev_len, dev_pos; int gpu_tried;
    struct bgzf_stager *stager;                         /* the stager thread's state (host_bgzf.c), while there is one */
    bgzf_rows_t rows;                                   /* the whole file's table, when the host has walked it */
    size_t g_nb, g_done;                                /* blocks in the file (when known), blocks decoded (under g_mu) */
    size_t dev_ready;                                   /* text bytes decoded so far (under g_mu) */
    size_t d_text_cap; int d_text_kind;
    void *d_tiles; size_t n_tiles, d_tiles_cap;                    /* the tokenizer's tile records of the decoded text, left by the CRC check (hpgv_bgzf_verify_tiles_dev) */
    size_t text_est;                                     /* about how much text the file holds (known when the stage has chosen its path) */
    int dev_len_known;                                  /* 0 while the stager is still finding the file's blocks (under g_mu) */
    void *d_scan;                                       /* the stager's slots (rows, statuses) and the device scan's scratch */
    int c_low;                                          /* cstream (and the slots' streams) have the lowest priority */
    pthread_t g_thread; pthread_mutex_t g_mu; pthread_cond_t g_cv; int g_started, g_sync, g_err, g_finished;
    /* the uploader: the compressed file goes up from the moment it is opened, beside the walk of its block headers */
    pthread_t u_thread; int u_started, u_cancel, u_err; size_t up_done;      /* bytes [0, up_done) are on the device (under g_mu) */
    /* a PART of a bgzip file staged on one member of a group context (bgzf_parts_stage): the bytes [file_off, file_off + size)
     * of the file, `map` pointing at its first byte, everything else as for a whole file.  ctx == NULL: an ordinary source */
    hpgv_ctx *ctx; int member; off_t file_off; int is_part;
    size_t map_len; const unsigned char *map_base;      /* the mapping as it was made (a part's is its file's) */
    struct src_parts *mp;                               /* the file's parts, when it is staged in parts (this source is part 0) */
} source_t;
/* the parts of one bgzip file, in file order; the reader walks them and joins the line that straddles two of them */
typedef struct src_parts {
    int n, cur;
    source_t *p[MEMBERS_MAX];                           /* p[0] = the reader's own source */
    char *seam; size_t seam_len, seam_cap;              /* the line across the seam in front of part `cur`, waiting to be handed out */
    off_t whole_size;
} src_parts_t;
#define SRC_CTX(s) ctx_use((s)->ctx, (s)->member)

enum { PREAD_SEG = 4 << 20, INFLATE_GROUP = 8, MAXB = 1 << 16 };

typedef struct {
    source_t src;
    char *carry; size_t carry_len, carry_cap;
    int eof;
    const char *last_dev;                               /* device copy of the batch read_lines just returned (BGZF on the GPU), or NULL */
    hpgv_ctx *last_ctx;                                 /* ... and the member context of that device when the file is staged in parts */
    const char *last_base; const void *last_tiles; size_t last_n_tiles;      /* ... where that device text begins, and its tile records */
    int devwin;                                         /* batches are windows of the device text; nothing but their cut points is read back */
    char *tailbuf; size_t tailcap;
    char *chrom_line; size_t chrom_len;                 /* the #CHROM line as written (vcf_header_read), or NULL */
} line_reader_t;

/* the file runners' tools.  The first two are the assoc tasks, as hpgv_assoc_text takes them */
/* RUN_CHISQ_PERM: the chi-square run with label permutation (hpgv_run_assoc_perm): RUN_CHISQ's file plus <out>.mperm;
 * RUN_TDT_PERM: the TDT run with family flips (hpgv_run_tdt_perm): RUN_TDT's file plus <out>.mperm;
 * RUN_MODEL / RUN_MODEL_PERM: the model tests (hpgv_run_assoc_model) without and with <out>.mperm of the trend statistic;
 * RUN_GENOME: sample relatedness (hpgv_run_genome): no line per record, one file of sample pairs written when the run ends;
 * RUN_GRM: the genetic relationship matrix (hpgv_run_grm): no line per record, three files written when the run ends;
 * RUN_LOGISTIC: the logistic regression with covariates (hpgv_run_assoc_logistic);
 * RUN_LINEAR: the linear regression of a quantitative trait with covariates (hpgv_run_assoc_linear) and, in a run with n_perms >= 1
 * (hpgv_run_assoc_linear_perm), the max(T) permutations of the reduced model's residuals: the same file plus <out>.mperm -- the one
 * tool whose .mperm is a property of the run, not of the table (run_mperm).
 * The stratified association (hpgv_run_assoc_cmh) is RUN_MODEL with a within file (run_cmh): the model run's cohort stage, filters,
 * sorting and per-line arrays -- one hpgv_cmh_result (nine doubles) in the model tests' ten per line -- with its own strata, engine call, header and line;
 * given n_perms >= 1 (hpgv_run_assoc_cmh_perm) it also writes <out>.mperm of CHISQ_CMH under labels shuffled within the strata, as the linear run does */
typedef enum { RUN_CHISQ = CHI_SQUARE, RUN_FISHER = FISHER, RUN_TDT, RUN_VCF2EPI, RUN_AGGREGATE, RUN_STATS, RUN_FILTER, RUN_SPLIT, RUN_CHISQ_PERM, RUN_TDT_PERM,
               RUN_MODEL, RUN_MODEL_PERM, RUN_GENOME, RUN_GRM, RUN_LOGISTIC, RUN_LINEAR } run_tool_t;
enum { RUN_N_TOOLS = RUN_LINEAR + 1 };                /* (index 0, the assoc task NONE, is no tool) */

/* What a tool is: one row per tool, the one place that lists tools by property (tool_of).  A switch over the tools stays only
 * where each does something of its own: engine_call, the cohort per stage, the line layouts.
 *   cohort      what run_cohort installs: all columns (hpgv_set_stats_cohort), the PED's cases and controls, its families, or the
 *               samples with a trait.  The second and the last install the assoc cohort themselves, and --inh-dom / --inh-rec scan
 *               that one -- under RUN_LINEAR every sample with a trait, as unaffected; the others get the PED's conditions for them
 *   covar       ... with the regressions' covariates;  needs_ped: refused without a PED (RUN_LINEAR: its entry asks for one or a phenotype file)
 *   rec_filters runs under hpgv_run_set_record_filters;  sorts: result file sorted afterwards, `header` its first line, kept for the order check
 *   mperm       <out>.mperm beside the file;  counts: the counters of hpgv_stats_text_groups;  lines: a line (vcf2epi: a row) per record
 *   pairs       adds to the run's per-device sample-pair buffers, files written when the run ends
 *   file        the tool whose result file, line for line, this one writes;  ints, dbls: elements per line of run_batch_t::ints, ::dbl */
typedef enum { COHORT_COLUMNS, COHORT_CASE_CONTROL, COHORT_FAMILIES, COHORT_TRAIT } cohort_stage_t;
typedef struct {
    const char *name; cohort_stage_t cohort;
    unsigned covar : 1, needs_ped : 1, rec_filters : 1, sorts : 1, mperm : 1, counts : 1, lines : 1, pairs : 1;
    run_tool_t file; int ints, dbls; const char *header;
} tool_traits_t;
#define HDR_CHISQ "#CHR\tPOS\tID\tA1\tC_A1\tC_U1\tF_A1\tF_U1\tA2\tC_A2\tC_U2\tF_A2\tF_U2\tOR\tCHISQ\tP-VALUE"
#define HDR_FISHER "#CHR\tPOS\tID\tA1\tC_A1\tC_U1\tF_A1\tF_U1\tA2\tC_A2\tC_U2\tF_A2\tF_U2\tOR\tP-VALUE"
#define HDR_TDT "#CHR\tPOS\tID\tA1\tA2\tT\tU\tOR\tCHISQ\tP-VALUE"
#define HDR_MODEL "#CHR\tPOS\tID\tA1\tA2\tAFF\tUNAFF\tCHISQ_GENO\tP_GENO\tCHISQ_TREND\tP_TREND\tCHISQ_ALLELIC\tP_ALLELIC\tCHISQ_DOM\tP_DOM\tCHISQ_REC\tP_REC"
#define HDR_LOGISTIC "#CHR\tPOS\tID\tA1\tA2\tNOBS\tBETA\tSE\tOR\tSTAT\tP\tITER"
#define HDR_LINEAR "#CHR\tPOS\tID\tA1\tA2\tNOBS\tBETA\tSE\tSTAT\tP"
#define HDR_CMH "#CHR\tPOS\tID\tA1\tA2\tNSTRATA\tCHISQ_CMH\tP_CMH\tOR_MH\tSE\tL95\tU95\tCHISQ_BD\tP_BD"
static const tool_traits_t g_tool_traits[RUN_N_TOOLS] = {
    /*                    name          cohort               cov ped rf srt mp cnt ln pr  file           ints dbls header */
    [RUN_CHISQ]      = { "chisq",      COHORT_CASE_CONTROL, 0, 1, 1, 1, 0, 0, 1, 0, RUN_CHISQ,      4, 3,  HDR_CHISQ },
    [RUN_FISHER]     = { "fisher",     COHORT_CASE_CONTROL, 0, 1, 1, 1, 0, 0, 1, 0, RUN_FISHER,     4, 3,  HDR_FISHER },
    [RUN_TDT]        = { "tdt",        COHORT_FAMILIES,     0, 1, 1, 1, 0, 0, 1, 0, RUN_TDT,        4, 3,  HDR_TDT },
    [RUN_VCF2EPI]    = { "vcf2epi",    COHORT_CASE_CONTROL, 0, 1, 1, 0, 0, 0, 1, 0, RUN_VCF2EPI,    4, 3,  NULL },
    [RUN_AGGREGATE]  = { "aggregate",  COHORT_COLUMNS,      0, 0, 1, 0, 0, 1, 1, 0, RUN_AGGREGATE,  4, 3,  NULL },
    [RUN_STATS]      = { "stats",      COHORT_COLUMNS,      0, 0, 0, 0, 0, 1, 1, 0, RUN_STATS,      4, 3,  NULL },
    [RUN_FILTER]     = { "filter",     COHORT_COLUMNS,      0, 0, 1, 0, 0, 0, 0, 0, RUN_FILTER,     4, 3,  NULL },
    [RUN_SPLIT]      = { "split",      COHORT_COLUMNS,      0, 0, 0, 0, 0, 0, 0, 0, RUN_SPLIT,      4, 3,  NULL },
    [RUN_CHISQ_PERM] = { "chisq_perm", COHORT_CASE_CONTROL, 0, 1, 1, 1, 1, 0, 1, 0, RUN_CHISQ,      4, 3,  HDR_CHISQ },
    [RUN_TDT_PERM]   = { "tdt_perm",   COHORT_FAMILIES,     0, 1, 1, 1, 1, 0, 1, 0, RUN_TDT,        4, 3,  HDR_TDT },
    [RUN_MODEL]      = { "model",      COHORT_CASE_CONTROL, 0, 1, 1, 1, 0, 0, 1, 0, RUN_MODEL,      8, 10, HDR_MODEL },
    [RUN_MODEL_PERM] = { "model_perm", COHORT_CASE_CONTROL, 0, 1, 1, 1, 1, 0, 1, 0, RUN_MODEL,      8, 10, HDR_MODEL },
    [RUN_GENOME]     = { "genome",     COHORT_COLUMNS,      0, 0, 0, 0, 0, 0, 0, 1, RUN_GENOME,     4, 3,  NULL },
    [RUN_GRM]        = { "grm",        COHORT_COLUMNS,      0, 0, 0, 0, 0, 0, 0, 1, RUN_GRM,        4, 3,  NULL },
    [RUN_LOGISTIC]   = { "logistic",   COHORT_CASE_CONTROL, 1, 1, 1, 1, 0, 0, 1, 0, RUN_LOGISTIC,   4, 6,  HDR_LOGISTIC },
    [RUN_LINEAR]     = { "linear",     COHORT_TRAIT,        1, 0, 1, 1, 0, 0, 1, 0, RUN_LINEAR,     4, 6,  HDR_LINEAR },
};
static inline const tool_traits_t *tool_of(run_tool_t t) { return &g_tool_traits[t]; }
static inline int tool_installs_assoc_cohort(run_tool_t t) { return tool_of(t)->cohort == COHORT_CASE_CONTROL || tool_of(t)->cohort == COHORT_TRAIT; }
static inline int tool_writer_thread(run_tool_t t) { return tool_of(t)->sorts || tool_of(t)->counts; }      /* its lines may go through a thread of their own */

typedef struct {
    struct run *run;                                     /* the run the batch belongs to */
    char *text; size_t text_cap;                         /* page-locked, taken from the cache when the batch is first filled */
    const char *dev_text;                                /* the same bytes on the device (BGZF decoded there), or NULL */
    hpgv_ctx *dev_ctx;                                   /* the member context of that device (a file staged in parts), or NULL */
    const char *dev_base; const void *dev_tiles; size_t dev_n_tiles;      /* where the decoded text begins on the device, and its tile records (or NULL) */
    size_t bytes; int max_lines, n_lines;
    uint64_t *line_off; uint32_t *field_off; int32_t *status;
    int32_t *ints; double *dbl;                          /* 4 (assoc) or 2 (tdt) int arrays, 3 double arrays; the model tests: counts8 per line, then
                                                          * chisq5 per line and, from dbl + 5 * max_lines, p5 per line; genome and grm: class4 per line in ints;
                                                          * logistic, linear: one hpgv_logistic_result / hpgv_linear_result (six doubles' room) per line in dbl; a model run with a
                                                          * within file (run_cmh): one hpgv_cmh_result per line in dbl, nine of the model tests' ten doubles */
    int32_t *n_ge; double *bmax;                         /* the permutation tools: permutations at or above the observed statistic per line; the batch's maximum per permutation */
    double *t_obs;                                       /* the linear run with permutations: the permuted statistic's observed value per line (the others' stands in ::dbl) */
    uint8_t *rows; size_t rows_cap; int row_width;       /* vcf2epi: one dataset row per line */
    int stats;                                           /* aggregate / stats: the counters of hpgv_stats_text */
    int32_t *c8, *merr, *midx, *mtab, *smiss, *cerr; double *hw;
    int n_multi, multi_cap, n_smiss, n_cerr;
    int n_groups; int32_t *gc8; double *ghw;              /* stats: per-phenotype counters, [g * max_lines + v] */
    uint8_t *keep; int keep_cap;                         /* filter: record_passes per line, then the partitioned text in `text` */
    uint64_t part_kept, part_total;                      /* ... its kept bytes first, part_total bytes in all */
    long n_pass, n_rej; int n_blank;                     /* ... records kept, records rejected, empty lines (in neither file) */
    int part_bgzf; uint8_t part_last[2];                 /* HPGV_OUT_BGZF: `text` holds the two parts' BGZF members (part_kept / part_total: their bytes); the parts' last text bytes */
    /* split: the bucket of every line in keep (SPLIT_NO_FILE: none), the line ranges of one hpgv_text_multisplit each, and per
     * bucket (over all ranges, in order) its split name and its bytes; the buckets' lines back to back in `text`.  n_pass:
     * records written, n_skip: lines that go to no file */
    int *sp_range; int sp_n_ranges, sp_range_cap;         /* per range: first line, lines, buckets */
    uint64_t *sp_len; int *sp_name; int sp_n_buckets, sp_bucket_cap;      /* per bucket: bytes, offset of its name in sp_names */
    char *sp_names; size_t sp_names_len, sp_names_cap;    /* the split names, NUL-terminated, back to back */
    /* HPGV_OUT_BGZF: sp_len's top bits say what a bucket's bytes are -- SP_MEMBERS: BGZF members (deflated on the device),
     * SP_NEEDS_NL: whose text lacks its last newline */
    long n_skip;
    /* clumping (run_t::clump): per line its number among the batch's candidates (p <= p2) or -1, and the candidates' genotype rows,
     * n_samples bytes each, as hpgv_assoc_select_text leaves them */
    int32_t *sel; uint8_t *crows; int crows_cap, n_sel;
} run_batch_t;

typedef struct { int na, miss_al, miss_gt, ac[15], gc[225]; } vcounts_t;

typedef struct { char *p; size_t len, cap; int disorder; } out_buf_t;

typedef struct { char *last; size_t cap; int have, disorder; } order_track_t;

typedef struct {
    pthread_mutex_t mu; pthread_cond_t cv; pthread_t th;
    FILE *fd; out_buf_t *bufs; int parts;              /* the set handed over (parts > 0), taken when the thread starts on it */
    int busy, stop, bad, started;
} file_writer_t;

typedef struct { const char *line; int neg1, order1; long double v1; int neg2; long double v2; } sort_key_t;

/* hpg-var-vcf stats: what the run accumulates besides the per-variant lines (sample_stats_t, file_stats_t) */
typedef struct {
    long *smiss, *serr;                                   /* per VCF column: missing genotypes, Mendelian errors as a child */
    long variants, biallelic, multiallelic, snps, indels, transitions, transversions, pass, with_quality;
    double quality_sum;
} run_stats_t;

/* hpg-var-vcf split: the output files, by lower-cased split name (host_vcftools.c) */
enum { SPLIT_OPEN_MAX = 64 };
#define SP_MEMBERS (1ull << 63)
#define SP_NEEDS_NL (1ull << 62)
#define SP_LEN(x) ((x) & ~(SP_MEMBERS | SP_NEEDS_NL))
typedef struct { char *name, *path; FILE *fd; long last; int created; } split_file_t;
typedef struct { split_file_t *f; int n, cap; sample_ids_t *ids; char *key; size_t key_cap; int open[SPLIT_OPEN_MAX], n_open; long clock; } split_files_t;

/* the parsed setting of hpgv_run_set_record_filters (host_records.c), shared by reference with the runs started under it */
typedef struct rec_filters rec_filters_t;

/* "CHR\tPOS\tID" of the records a side output keeps, in file order: n of them, NUL-terminated in the arena `heads`, head[i] the
 * offset of record i's (host_sideout.c: rec_heads_*).  The arrays a store keeps beside it have H.cap elements, as head has */
typedef struct { size_t *head; size_t n, cap; char *heads; size_t heads_len, heads_cap; } rec_heads_t;

/* the permutation tools (tool_traits_t::mperm): what the run keeps for <out>.mperm -- the maxima merged over the batches (by the engine threads, under the
 * pipeline's mutex) and, per written record in file order, "CHR\tPOS\tID", the observed statistic and its n_ge */
typedef struct { double *tmax; double *t_obs; int32_t *n_ge; rec_heads_t H; } run_perm_t;

/* clumping (hpgv_run_assoc_clump): the run's candidate store -- per written record with p <= p2, in file order, its genotype row
 * (n_samples bytes), its p, its chromosome (numbered in order of first appearance) and position, and "CHR\tPOS\tID" */
typedef struct {
    uint8_t *rows; double *p; int32_t *chrom; uint32_t *pos; rec_heads_t H;
    char **chrom_names; int n_chroms, chrom_cap;
    long n_clumps, n_truncated;
} run_clump_t;

/* sample relatedness (hpgv_run_genome): one n_samples x n_samples buffer of pair counts per device of the run, zeroed when the
 * run starts, which the batches' hpgv_ibs_text calls add to (a batch goes to the device that holds its text, else the devices take
 * turns); the terms of the written records that are used, added in file order by the writer loop, and their number */
typedef struct {
    int n_dev; hpgv_ctx **ctx; hpgv_ibs_counts **d_counts;
    unsigned next;
    double sum[5]; long used;
    long n_pairs;                                        /* pairs written to the file */
} run_genome_t;

/* allele scoring (hpgv_run_score): the score file -- n lines of id, allele and n_scores weights, the ids in an open-addressing hash
 * (slot: a line or -1) --, the scale of every column, and the records whose allele matched neither REF nor ALT, counted by the
 * engine threads.  The strings lie in blob */
typedef struct {
    int n_scores, impute, have_header; int frac_bits[HPGV_SCORE_MAX];
    long n; char **id, **allele; double *w; long *slot; size_t mask; char *blob;
    char (*name)[64];                                    /* the columns' names */
    long n_unmatched;
} run_score_t;

/* the covariate file of the logistic run (host_covar.c): n lines of ncols value columns, iid[i] the line's second id (in blob),
 * val[i * ncols + k] NaN where the text is not a finite number */
typedef struct { int n, ncols, ncols_set; char **iid, **c1; double *val; char *blob; } covar_table_t;      /* c1[i]: the first value column's text (the within file's cluster name), or NULL */

/* one file run: built by its public entry (hpgv_run_*), its stages and the pipeline's threads (through the batches) share it */
typedef struct run {
    run_tool_t tool;
    hpgv_run_filters_t filters;                          /* the record filters as the run started (stats, split: all off) */
    rec_filters_t *rf;                                   /* ... and those of hpgv_run_set_record_filters (NULL: all off), held by run_file */
    int overwrite, save_rejected;                        /* aggregate: AC / AF / AN replaced; filter: the others to .rejected */
    int out_bgzf;                                        /* filter, split: hpgv_run_set_output_compression as the run started */
    int criterion, n_iv; const long *iv; const char *dir; char base[512];  /* split: HPGV_SPLIT_*, coverage bounds, <dir>/<name>_<base> */
    long written, rejected;                              /* records written; filter: records written to (or meant for) .rejected */
    long files, skipped, key_ns;                         /* split: files created, lines to no file, host time of split_keys */
    line_reader_t rd; char *hdr, **names; size_t chrom_off; int n_samples, io_threads, n_engines; ped_table_t ped;
    int n_trios, n_groups; int32_t *trio_child; char **group_names;     /* stats: trios' child columns, phenotypes (PED text) */
    uint32_t epi_aff, epi_unaff;                         /* vcf2epi: the class sizes */
    char *path, *path_rej; FILE *out, *out_rej, **gfd;   /* gfd: stats, one file per phenotype */
    split_files_t SF; run_stats_t *RS; order_track_t ord;
    int n_perms; uint64_t perm_seed; run_perm_t *PM;      /* the permutation tools */
    const hpgv_run_clump_options_t *clump; run_clump_t *CL;      /* RUN_CHISQ / RUN_FISHER with <out>.clumped beside the file (NULL: without) */
    long n_clumps, n_truncated;                          /* ... what run_clump_write counted, kept past the store */
    double min_pi_hat; run_genome_t *GN; long n_pairs;   /* RUN_GENOME: the threshold, the run's counts, the pairs written (kept past them) */
    double min_maf; int frac_bits;                       /* RUN_GRM: the rows' rule and hpgv_grm_frac_bits of it; its sums lie in GN's buffers (16-byte records too) */
    int n_pcs, write_grm, n_iter;                        /* RUN_GRM with n_pcs >= 1 (hpgv_run_pca): pairs to write, the .grm.* files too, the sweeps done (kept past the run) */
    run_score_t *score;                                  /* RUN_GRM with a score plan (hpgv_run_score): GN's buffers hold the score sums, the run ends in a .profile */
    const covar_table_t *covar; int n_covar; long n_used; /* RUN_LOGISTIC, RUN_LINEAR: the covariate file (NULL: none) and its columns in use; the cohort samples that stayed */
    const covar_table_t *pheno;                          /* RUN_LINEAR: the phenotype file (NULL: the PED's sixth column) */
    const covar_table_t *within; int n_strata;           /* RUN_MODEL as the stratified association: the within file; the strata among the cohort that stayed */
    double t_opened, t_header, t_sort;
} run_t;
/* the run writes <out>.mperm: the permutation tools of the table, and the linear run and the stratified association when they are
 * given permutations */
/* the run is the stratified association: the model tool with a within file */
static inline int run_cmh(const run_t *R) { return R->tool == RUN_MODEL && R->within != NULL; }
static inline const char *run_header(const run_t *R) { return run_cmh(R) ? HDR_CMH : tool_of(R->tool)->header; }
static inline int run_mperm(const run_t *R) { return tool_of(R->tool)->mperm || ((R->tool == RUN_LINEAR || run_cmh(R)) && R->n_perms > 0); }

enum { RUN_ENGINES_MAX = 16, RUN_NB_MAX = RUN_ENGINES_MAX + 3, RUN_FMT_BUFS = 64 };

/* what the current device-side cohort descriptions were built from */
struct host_assoc_key {
    const void *samples; int num_samples; uint64_t cond_hash; int set;
    uint8_t *cond;                                       /* the installed condition vector itself: a hash hit is confirmed against it */
};
extern struct host_assoc_key g_assoc_key;
struct host_tdt_key {
    int num_families; int num_columns; uint64_t hash; int set;
    int32_t *csr; uint8_t *csex; size_t n_children;       /* the installed description itself (father | mother | offsets | child columns): a hash hit is confirmed against it */
};
extern struct host_tdt_key g_tdt_key;
struct host_stats_key { int num_samples; int set; };
extern struct host_stats_key g_stats_key;
struct host_ped_key { int num_samples; int n_trios; uint64_t hash; int set; };
extern struct host_ped_key g_ped_key;
struct host_group_key { int num_samples; int n_groups; uint64_t hash; int set; };
extern struct host_group_key g_group_key;
struct host_lf_key { const void *table; int n; };
extern struct host_lf_key g_lf_key;

/* The environment of libhpgv_host.so (include/hpgv_host.h "Environment"): read by host_env_read() when the engine is bound and
 * at the start of every file run -- never on a per-batch or per-block path -- into this one structure. */
typedef struct {
    long devices_set;                /* HPGV_DEVICES given (its text is parsed by the engine binding) */
    long io_threads;                 /* HPGV_IO_THREADS: reader / formatter team (0: by the cores) */
    long stage_threads;              /* HPGV_STAGE_THREADS: team of a lone adapter caller's staging (0: 8) */
    long engine_threads;             /* HPGV_ENGINE_THREADS: batches in flight on the devices (0: by the input) */
    long run_trace;                  /* HPGV_RUN_TRACE=1: stage times of a run on stderr */
    long bgzf_verify;                /* HPGV_BGZF_VERIFY=0: no CRC-32 check of decoded blocks (default 1) */
    long zlib_inflate;               /* HPGV_ZLIB_INFLATE=1: host blocks through zlib instead of the built-in decoder */
    long no_gpu_inflate;             /* HPGV_NO_GPU_INFLATE=1: bgzip decoded on the host */
    long no_device_windows;          /* HPGV_NO_DEVICE_WINDOWS=1: device-decoded text copied back whole */
    long no_large_windows;           /* HPGV_NO_LARGE_WINDOWS=1: windows of the caller's batch size */
    long bgzf_one_device;            /* HPGV_BGZF_ONE_DEVICE=1: a group decodes the file on member 0 only */
    long bgzf_host_table;            /* HPGV_BGZF_HOST_TABLE=1: the block table walked by the host's team */
    long serial_bgzf_walk;           /* HPGV_SERIAL_BGZF_WALK=1: ... by one thread */
    long no_growing_text;            /* HPGV_NO_GROWING_TEXT=1: a fixed device buffer for the decoded text */
    long no_low_priority;            /* HPGV_NO_LOW_PRIORITY=1: the decoder's streams at normal priority */
    long no_decode_tiles;            /* HPGV_DECODE_TILES=0: the CRC check leaves no tile records (windows tokenized with the counting sweep) */
    long no_numa_bind;               /* HPGV_NO_NUMA_BIND=1: a run's threads stay where the scheduler puts them */
    long no_writer_thread;           /* HPGV_NO_WRITER_THREAD=1: result lines written by the formatting thread */
    long always_sort;                /* HPGV_ALWAYS_SORT=1: the output is sorted even when it came out in order */
    long upload_segment_mb;          /* HPGV_UPLOAD_SEGMENT_MB (1..64, default 4), upload_inflight: HPGV_UPLOAD_INFLIGHT (1..8, default 2) */
    long upload_inflight;
    /* tests only */
    long test_refuse_every;          /* HPGV_TEST_GPU_INFLATE_REFUSE_EVERY: every n-th block handed back to the host decoder */
    long test_damage_every;          /* HPGV_TEST_GPU_INFLATE_DAMAGE_EVERY: every n-th block's decoded text overwritten in its middle before the CRC check */
    long test_scan_rows;             /* HPGV_TEST_SCAN_ROWS: no stretch of the stager longer than this many blocks */
    long test_text_estimate_percent; /* HPGV_TEST_TEXT_ESTIMATE_PERCENT: the first commitment as a share of the estimate */
    long bgzf_part_min_kb;           /* HPGV_BGZF_PART_MIN_KB: smallest part of a file staged in parts (default 65536) */
} host_env_t;
extern host_env_t g_env;
void host_env_read(void);

/* ---- functions and data the units share ---- */
/* host_containers.c */
void list_insert_chain(list_item_t *first, list_item_t *last, size_t n, list_t *list);
/* host_pool.c */
void pool_init(io_pool_t *p, int n_threads);
void pool_spread(io_pool_t *p);
void pool_destroy(io_pool_t *p);
void pool_run(io_pool_t *p, pool_fn fn, void *arg, int n_tasks);
int default_io_threads(void);
int numa_bind_to_device(cpu_set_t *saved);
void numa_unbind(const cpu_set_t *saved, int bound);
/* host_stage.c */
void stage_team_release(void);
/* host_engine.c */
int host_fail(const char *what, int rc);
char *text_buf_get(size_t cap);
void text_buf_put(char *p, size_t cap);
uint8_t *stage_get(size_t bytes, int *slot);
void stage_put(uint8_t *p, int slot);
void dev_text_free(void *p, int kind);
void *dev_text_get(size_t bytes, size_t *cap, int *kind);
int dev_text_grow(void *p, size_t bytes, size_t *cap);
void dev_text_drop_cached(void);
void dev_text_put(void *p, size_t bytes, int kind);
void *dev_tiles_get(size_t bytes, size_t *cap);
void dev_tiles_put(void *p, size_t cap);
int stream_get(int low, void **out);
void stream_put(int low, void *st);
int ensure_engine(void);
char *dupn(const char *s, int n);
int thread_id(void);
/* host_output.c */
void make_key(const char *line, sort_key_t *k);
int cmp_keys(const void *pa, const void *pb);
/* host_source.c */
void ped_table_free(ped_table_t *p);
int ped_table_read(const char *path, ped_table_t *ped);
double now_s(void);
int bgzf_block(const unsigned char *p, size_t avail, size_t *bsize, size_t *cdata_off, size_t *isize);
int source_open(source_t *s, const char *path);
void source_close(source_t *s);
void source_task_pread(void *v, int k);
void source_task_inflate(void *v, int g);
/* host_inflate.c */
int fast_inflate(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_len);
int inflate_block(const unsigned char *in, size_t clen, unsigned char *out, size_t isize);
/* host_bgzf.c */
int bgzf_rows_reserve(bgzf_rows_t *t, size_t cap);       /* room for cap rows; 0 = no memory */
void bgzf_rows_free(bgzf_rows_t *t);
int bgzf_walk_parallel(int fd, size_t size, bgzf_rows_t *t, size_t *text);      /* the whole file's table by a team; non-zero: walk serially */
int bgzf_walk_serial(const unsigned char *map, size_t size, bgzf_rows_t *t, size_t *text);
int bgzf_gpu_stage(source_t *s);
void upload_cancel(source_t *s);
void bgzf_stage_release(source_t *s);
/* host_reader.c */
size_t read_lines_dev(line_reader_t *r, char *buf, size_t bufcap, size_t cap);
size_t read_lines(line_reader_t *r, char *buf, size_t cap);
int vcf_header_read(line_reader_t *rd, char **hdr_out, char ***names_out, size_t *chrom_off);
/* host_format.c */
int run_batch_alloc(run_batch_t *b, run_t *run, size_t cap_bytes, int n_samples, int n_trios, int n_groups);
int run_batch_reserve(run_batch_t *b, int lines);
void run_batch_free(run_batch_t *b);
int record_passes(const run_batch_t *b, int i);
void record_counts(const run_batch_t *b, int i, const char *alt, int la, vcounts_t *v);
void order_track_keep(order_track_t *o, const char *line, size_t len);
int file_writer_start(file_writer_t *w, FILE *fd);
int file_writer_stop(file_writer_t *w);
int write_batch(FILE *fd, const run_batch_t *b, out_buf_t *bufs, int n_bufs, io_pool_t *pool, order_track_t *ord, file_writer_t *fw);
/* host_sideout.c: per side output, _new in run_outputs, _add per written batch, _write and _free (which clears the run's pointer) in run_finish */
int rec_heads_init(rec_heads_t *H, size_t first_cap);    /* head allocated for first_cap records, doubled from there; these two: non-zero = no memory */
int rec_heads_add(rec_heads_t *H, const char *chr, int lc, long pos, const char *id, int li);
const char *rec_heads_get(const rec_heads_t *H, size_t i);
void rec_heads_free(rec_heads_t *H);
int run_perm_new(run_t *R);
int run_perm_add(run_t *R, const run_batch_t *b);        /* the _adds of .mperm and .clumped: non-zero = no memory */
int run_perm_write(run_t *R, const char *out_path);
void run_perm_free(run_t *R);
int run_clump_new(run_t *R);
int run_clump_add(run_t *R, const run_batch_t *b);
int run_clump_write(run_t *R, const char *out_path);
void run_clump_free(run_t *R);
int run_genome_new(run_t *R);                            /* an hpgv status, the message in g_err */
hpgv_ctx *run_genome_device(run_t *R, const run_batch_t *b, hpgv_ibs_counts **d_counts);      /* the context and buffer a batch's engine call uses */
void run_genome_add(run_t *R, const run_batch_t *b);     /* and the run's count of records that took part */
int run_genome_write(run_t *R, const char *out_path);
void run_genome_free(run_t *R);
void run_grm_add(run_t *R, const run_batch_t *b);        /* the run's count of USED records */
int run_grm_write(run_t *R, const char *out_prefix);
int run_grm_sum(run_t *R, hpgv_grm_acc **sum_out);       /* the devices' records added on the host; run_grm_files: the three files of the sum */
int run_grm_files(run_t *R, const char *out_prefix, const hpgv_grm_acc *sum);
int grm_put(const char *prefix, const char *suffix, const void *data, size_t bytes);      /* <prefix><suffix> written whole */
int run_score_read(const char *path, int impute, run_score_t *S);      /* the score file; run_score_free: what it allocated */
void run_score_free(run_score_t *S);
int run_score_weigh(void *user, const char *text, int n_lines, const uint64_t *line_off, const uint32_t *field_off, const int32_t *status,
                    double *w, uint8_t *flags);          /* hpgv_score_text's callback, user: the run's run_score_t */
size_t run_score_acc_pitch(const run_t *R);              /* int64 per plane of a device's sums; the constants lie behind the n_scores + 2 planes */
int run_score_sum(run_t *R, int64_t **sum_out);          /* the devices' sums and constants added on the host; run_score_write: the .profile of them */
int run_score_write(run_t *R, const char *out_path);
int run_pca_write(run_t *R, const char *out_prefix);     /* host_pca.c: the GRM run's end when principal components are asked for */
int run_stats_new(run_t *R);
void run_stats_add(run_t *R, const run_batch_t *b);      /* and the batch's lines to the per-phenotype files */
int run_stats_write(const run_t *R, const char *prefix);
void run_stats_free(run_t *R);
/* host_covar.c */
int covar_table_read(const char *path, covar_table_t *T);      /* these: an hpgv status, the message in g_err */
int covar_table_columns(const covar_table_t *T, int n_covar);  /* the columns a run uses, or -1 */
int covar_table_match(const covar_table_t *T, char *const *names, int n, int use, double *cov, size_t stride, uint8_t *have);
void covar_table_free(covar_table_t *T);
int within_table_read(const char *path, covar_table_t *T);     /* the within file: one value column, the cluster's name */
int within_table_match(const covar_table_t *T, char *const *names, int n, const uint8_t *take, int32_t *stratum, int *n_strata);
/* host_vcftools.c */
int filter_partition(run_batch_t *b);
int split_partition(run_batch_t *b);
int write_filter_header(FILE *f, const run_t *R);
int write_filter_batch(FILE *kept, FILE *rejected, const run_batch_t *b);
int write_split_batch(run_t *R, const run_batch_t *b);
int split_files_close(split_files_t *S, int bgzf);
int out_compression_now(void);                           /* the setting of hpgv_run_set_output_compression */
size_t out_batch_cap(const struct run *R, size_t batch_bytes);      /* room a batch's buffer needs for what the tool's engine step leaves in it */
int bgzf_write_eof(FILE *f);

/* host_records.c */
int info_dp(const char *info, size_t n, long long *v);
int record_info(const run_batch_t *b, int i, const char **info, size_t *n);
rec_filters_t *rec_filters_take(void);                   /* the current setting, referenced (NULL: all off) */
void rec_filters_put(rec_filters_t *r);
const hpgv_run_record_filters_t *rec_filters_of(const rec_filters_t *r);
int rec_filters_inheritance(const rec_filters_t *r);     /* --inh-dom or --inh-rec is set */
int rec_filters_pass(const rec_filters_t *r, const run_batch_t *b, int i);
void rec_filters_header(FILE *f, const rec_filters_t *r);

extern pthread_rwlock_t g_cohort_lock;   /* host_engine.c */
extern char g_err[512];   /* host_engine.c */
extern hpgv_run_filters_t g_filters;   /* host_source.c */
extern double g_run_times[6];   /* host_source.c */
extern char g_input_err[192];   /* host_inflate.c */
extern double g_write_split[2];   /* host_format.c */

#pragma GCC visibility pop
#endif
