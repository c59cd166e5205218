/*
 * hpgv_host.h -- host-side mirror of the reference's per-batch runner API.
 *
 * hpg-variant's runners call three C functions once per parsed VCF batch
 * (SURVEY.md 8b).  This header gives those functions with the reference's own
 * names, argument order, ownership and error behaviour, re-hosted on the
 * MI355X engine (include/hpgv.h).  The hpg-libs types they take are not in the
 * reference tree (lib/ is an empty submodule), so the few fields the hot path
 * touches are defined here with the reference's field names:
 *
 *   assoc_test          src/gwas/assoc/assoc.h:137-138   (body assoc.c:23-84)
 *   tdt_test            src/gwas/tdt/tdt.h:119           (body tdt.c:23-276)
 *   get_variants_stats  call site src/vcf-tools/stats/stats_runner.c:194-195
 *   result records      assoc_basic_test.h:30-46, assoc_fisher_test.h:29-44, tdt.h:104-117
 *   writers             assoc_runner.c:292-342, tdt_runner.c:286-304
 *
 * What the adapters do per call: find GT in FORMAT, turn every sample string
 * into one HPGV8 byte (the reference's strdup + get_alleles per genotype,
 * assoc.c:45-56), hand the batch to the engine, and build one result record
 * per variant on the caller's list_t, stamped with the OpenMP thread id
 * (assoc.c:25,67-68).  No statistics are computed on the host.
 */
#ifndef HPGV_HOST_H
#define HPGV_HOST_H

#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "hpgv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- hpg-libs stand-in types (only what the hot path reads) ---------------- */

typedef struct array_list {            /* containers/array_list.h: items, size */
    size_t capacity;
    size_t size;
    void **items;
} array_list_t;

array_list_t *array_list_new(size_t initial_capacity);
int   array_list_insert(void *item, array_list_t *list);
void *array_list_get(size_t index, const array_list_t *list);
void  array_list_free(array_list_t *list, void (*item_free)(void *));

typedef struct vcf_record {            /* bioformats/vcf/vcf_file_structure.h; fields as used in
                                          assoc.c:40-65, tdt.c:43-48,262-266 */
    char *chromosome;  int chromosome_len;
    unsigned long position;
    char *id;          int id_len;
    char *reference;   int reference_len;
    char *alternate;   int alternate_len;
    char *format;      int format_len;
    array_list_t *samples;             /* NUL-terminated per-sample strings "0/1:..." */
} vcf_record_t;

vcf_record_t *vcf_record_new(void);
void vcf_record_free(vcf_record_t *record);          /* frees the record and its samples list, not the strings */
void set_vcf_record_chromosome(char *chromosome, int length, vcf_record_t *record);
void set_vcf_record_position(long position, vcf_record_t *record);
void set_vcf_record_id(char *id, int length, vcf_record_t *record);
void set_vcf_record_reference(char *reference, int length, vcf_record_t *record);
void set_vcf_record_alternate(char *alternate, int length, vcf_record_t *record);
void set_vcf_record_format(char *format, int length, vcf_record_t *record);

enum Sex { MALE = HPGV_SEX_MALE, FEMALE = HPGV_SEX_FEMALE, UNKNOWN_SEX = HPGV_SEX_UNKNOWN };
enum Condition { UNAFFECTED = HPGV_COND_UNAFFECTED, AFFECTED = HPGV_COND_AFFECTED,
                 MISSING_CONDITION = HPGV_COND_OTHER };

struct family;
typedef struct individual {            /* bioformats/family/family.h; ctor shape from
                                          test/test_tdt_runner.c:95-97 */
    char *id;
    float variable;
    enum Sex sex;
    enum Condition condition;
    struct individual *father;
    struct individual *mother;
    struct family *family;
} individual_t;

individual_t *individual_new(char *id, float variable, enum Sex sex, enum Condition condition,
                             individual_t *father, individual_t *mother, struct family *family);
void individual_free(individual_t *individual);

/* family->founders / family->members are khashes in the reference (tdt.c:62-66,
 * 135-137); here they are ordered lists, iterated in insertion order. */
typedef struct family {
    char *id;
    array_list_t *founders;            /* individual_t*, parents without parents */
    array_list_t *members;             /* individual_t*, everybody else */
} family_t;

family_t *family_new(char *id);
int  family_set_parent(individual_t *parent, family_t *family);
int  family_add_child(individual_t *child, family_t *family);
void family_free(family_t *family);    /* frees the lists, not the individuals */

/* khash_t(ids): sample name -> VCF column (tdt.c:83-95); open addressing, strings borrowed */
typedef struct sample_ids {
    size_t n_buckets;
    size_t size;
    const char **keys;
    int *vals;
} sample_ids_t;

sample_ids_t *sample_ids_new(size_t expected);
int  sample_ids_put(sample_ids_t *ids, const char *name, int position);
int  sample_ids_get(const sample_ids_t *ids, const char *name);   /* -1 when absent */
void sample_ids_free(sample_ids_t *ids);

/* containers/list.h: thread-safe producer/consumer list (assoc_runner.c:25,306; assoc.c:67-68) */
typedef struct list_item {
    int id;
    int type;
    void *data_p;
    struct list_item *next_p;
} list_item_t;

typedef struct list {
    char *name;
    int writers;
    size_t max_length;
    size_t length;
    list_item_t *first_p, *last_p;
    pthread_mutex_t lock;
    pthread_cond_t condition;
} list_t;

void list_init(const char *name, int writers, size_t max_length, list_t *list);
list_item_t *list_item_new(int id, int type, void *data_p);
void list_item_free(list_item_t *item);
int  list_insert_item(list_item_t *item, list_t *list);
list_item_t *list_remove_item(list_t *list);   /* blocks while empty and writers > 0; NULL at the end */
int  list_decr_writers(list_t *list);
void list_free_deep(list_t *list, void (*data_free)(void *));

/* ---- result records: field for field the reference's ----------------------- */

enum ASSOC_task { NONE = HPGV_TASK_NONE, CHI_SQUARE = HPGV_TASK_CHISQ, FISHER = HPGV_TASK_FISHER };

typedef struct {                       /* assoc_basic_test.h:30-46 */
    char *chromosome; char *id; char *reference; char *alternate;
    unsigned long int position;
    int affected1, affected2, unaffected1, unaffected2;
    double odds_ratio, chi_square, p_value;
} assoc_basic_result_t;

typedef struct {                       /* assoc_fisher_test.h:29-44 */
    char *chromosome; char *id; char *reference; char *alternate;
    unsigned long int position;
    int affected1, affected2, unaffected1, unaffected2;
    double odds_ratio, p_value;
} assoc_fisher_result_t;

typedef struct {                       /* tdt.h:104-117 */
    char *chromosome; char *id; char *reference; char *alternate;
    unsigned long int position;
    int t1, t2;
    double odds_ratio, chi_square, p_value;
} tdt_result_t;

void assoc_basic_result_free(assoc_basic_result_t *result);
void assoc_fisher_result_free(assoc_fisher_result_t *result);
void tdt_result_free(tdt_result_t *result);

/* variant_stats_t: the fields visible in the reference tree
 * (aggregate_runner.c:187-191,288-312,379-400), plus the Hardy-Weinberg record the
 * stats tool reports.  Arrays are sized by num_alleles (1 + number of ALT alleles). */
typedef struct {                       /* the counters of one phenotype group (first two alleles) */
    int alleles_count[2];
    int genotypes_count[4];            /* 0/0, 0/1, 1/0, 1/1 */
    float alleles_freq[2];
    int missing_alleles, missing_genotypes;
    float maf;
    double hw_chi2, hw_p_value;
} variant_phenotype_stats_t;

typedef struct {
    char *chromosome; unsigned long position;
    char *ref_allele; char *alt_alleles;
    int num_alleles;
    int *alleles_count;                /* [num_alleles] */
    int *genotypes_count;              /* [a1 * num_alleles + a2] */
    float *alleles_freq;
    float *genotypes_freq;
    int missing_alleles, missing_genotypes;
    float maf;
    double hw_chi2, hw_p_value;        /* on the first two alleles */
    int num_phenotypes;                /* num_variables of the call (0 without a PED) */
    variant_phenotype_stats_t *phenotype_stats;   /* [num_phenotypes]: samples whose individual->variable is that id
                                          (report_vcf_variant_phenotype_stats(fd, n, batch, i), stats_runner.c:319-323) */
} variant_stats_t;

void variant_stats_free(variant_stats_t *stats);

typedef struct {                       /* sample_stats_t (stats_runner.c:158-160): per-sample counters */
    char *name;
    int missing_genotypes;
    int mendelian_errors;              /* variants at which the sample, as a child, contradicts its parents */
} sample_stats_t;

sample_stats_t *sample_stats_new(char *name);
void sample_stats_free(sample_stats_t *stats);

typedef struct {                       /* file_stats_t: summary counters (simple sums) */
    int variants_count, samples_count, biallelics_count, multiallelics_count;
    pthread_mutex_t lock;
} file_stats_t;

file_stats_t *file_stats_new(void);
void file_stats_free(file_stats_t *stats);

/* ---- engine binding ---------------------------------------------------------- */
/* Chooses the device the adapters run on (default 0).  Called lazily by the
 * adapters; returns HPGV_OK or an hpgv status.  There is no CPU fallback. */
int  hpgv_host_init(int device_id);
/* several devices (hpgv_create_multi of include/hpgv.h): the adapters' and runners' batches are dealt to them; the
 * runners start two engine threads per device.  Without an explicit init the first call reads the environment variable
 * HPGV_DEVICES ("0,1,2,3" or "all"; the same id may repeat) and falls back to device 0. */
int  hpgv_host_init_devices(const int *device_ids, int n_devices);
int  hpgv_host_device_count(void);                     /* devices behind the adapters (0 before the first call) */
void hpgv_host_shutdown(void);
const char *hpgv_host_last_error(void);

/* ---- the reference's per-batch functions ------------------------------------- */

/* assoc.h:137-138.  void like the reference: an engine failure is logged to
 * stderr and exits the process with 1, which is what LOG_FATAL does there. */
void assoc_test(enum ASSOC_task test_type, vcf_record_t **variants, int num_variants,
                individual_t **samples, int num_samples,
                const void *opt_input, list_t *output_list);

/* assoc_runner.c:164-166 builds opt_input with init_logarithm_array(num_samples * 10) */
double *init_logarithm_array(int n);

/* tdt.h:119.  0 = OK (tdt_runner.c:186-188 treats non-zero as fatal). */
int  tdt_test(vcf_record_t **variants, int num_variants, family_t **families, int num_families,
              sample_ids_t *sample_ids, list_t *output_list);

/* call shape of stats_runner.c:194-195; returns 0 on success.  With individuals != NULL and
 * num_variables > 0 every record also carries the counters of each phenotype group: VCF column j
 * belongs to group (int)individuals[j]->variable when that is in [0, num_variables). */
int  get_variants_stats(vcf_record_t **variants, int num_variants, individual_t **individuals,
                        sample_ids_t *sample_ids, int num_variables, list_t *output_list,
                        file_stats_t *file_stats);

/* call shape of stats_runner.c:197-198; accumulates into sample_stats[j] for VCF column j */
int  get_sample_stats(vcf_record_t **variants, int num_variants, individual_t **individuals,
                      sample_ids_t *sample_ids, sample_stats_t **sample_stats, file_stats_t *file_stats);

/* ---- writers with the reference's exact formats ------------------------------ */
void assoc_write_output_header(enum ASSOC_task task, FILE *fd);             /* assoc_runner.c:292-299 */
void assoc_write_output_body(enum ASSOC_task task, list_t *output_list, FILE *fd);   /* :301-342 */
void tdt_write_output_header(FILE *fd);                                     /* tdt_runner.c:286-289 */
void tdt_write_output_body(list_t *output_list, FILE *fd);                  /* tdt_runner.c:291-304 */

/* In-process replacement of the runners' `system("sort -k1,1h -k2,2n FILE > FILE.tmp && mv ...")`
 * (assoc_runner.c:255-258, tdt_runner.c:255-261): sorts the lines of `path` (header included, as
 * the reference does) by column 1 "human numeric", then column 2 numeric, then the whole line
 * bytewise -- the order GNU sort gives under LC_ALL=C.  Returns 0, or non-zero when the file
 * cannot be read / rewritten (the reference only warns in that case). */
int  hpgv_host_sort_output_file(const char *path);

/* The characters of printf("%6f", x) -- the number format of the result files (assoc_runner.c:314-318,
 * tdt_runner.c:297-299) -- written to dst (room for 320 characters: the largest double takes 316); returns their count.  Rounds half to
 * even on the exact binary value, as glibc does; used by the file runners' writers in place of printf. */
int  hpgv_host_format_f6(double x, char *dst);

/* The runners' own raw-DEFLATE decoder for BGZF blocks (`--compression bgzip`, shared_options.c:60-61): `in` -> exactly
 * out_len bytes.  0 = decoded; non-zero = something the fast path does not take (the runners then let zlib decode and
 * judge the block).  Exported for the tests. */
int  hpgv_host_inflate_raw(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_len);

/* ---- file level: what run_association_test (assoc_runner.c:23-276) and run_tdt_test
 *      (tdt_runner.c:23-279) do, minus options/filters: read the PED, read the VCF (plain text,
 *      gzip or bgzip -- `--compression`, shared_options.c:60-61; detected from the file's magic, BGZF
 *      blocks are inflated in parallel) in text batches of about batch_bytes, hand every batch to the engine as TEXT (the GPU
 *      tokenizes it), write the reference's TSV and sort it in process.  (A bgzip file of 256 blocks or more is decoded on the
 *      device and its text stays there: batch_bytes is then a lower bound, the windows are about a 64th of the text, 256 MB
 *      at most.)  Reader, engine and
 *      writer overlap (one batch in flight each way).  PED columns: FID IID PAT MAT SEX PHENO
 *      with SEX 1 = male, 2 = female and PHENO 2 = affected, 1 = unaffected
 *      (stats_runner.c:50,86-87).  Returns 0 or an hpgv / errno-style non-zero code;
 *      *n_variants_out (may be NULL) receives the number of records written. */
int  hpgv_run_assoc(const char *vcf_path, const char *ped_path, const char *out_path,
                    enum ASSOC_task task, size_t batch_bytes, long *n_variants_out);
int  hpgv_run_tdt(const char *vcf_path, const char *ped_path, const char *out_path,
                  size_t batch_bytes, long *n_variants_out);
/* hpgv_run_assoc(..., CHI_SQUARE, ...) with max(T) label permutation (include/hpgv.h "label permutation"; PLINK's --mperm):
 * out_path is written byte for byte as there, and <out_path>.mperm beside it: the header line "#CHR\tPOS\tID\tEMP1\tEMP2",
 * then one line per written variant in the same sorted order -- EMP1 the pointwise empirical p-value, EMP2 the family-wise
 * one from the per-permutation maximum over every record of the file the engine scanned (a record that only a host-side field
 * filter drops still takes part; lines the engine's own record filters reject do not); numbers as hpgv_host_format_f6 prints them
 * (NaN as in the result file).  The n_perms label rows are generated once per run by hpgv_perm_labels_shuffle(seed) from the
 * PED's conditions; every batch goes through hpgv_assoc_perm_text and its maxima are merged into the run's by element-wise
 * maximum, so the result depends neither on batch_bytes nor on the number of engine threads or devices.  Same cohort, filters,
 * record filters and input forms (plain, gzip, bgzip) as hpgv_run_assoc.  n_perms < 1 or a NULL path: HPGV_ERR_INVALID before
 * the engine is started, and no file is written. */
int  hpgv_run_assoc_perm(const char *vcf_path, const char *ped_path, const char *out_path, int n_perms, uint64_t seed,
                         size_t batch_bytes, long *n_variants_out);
/* The model tests of a case/control scan (include/hpgv.h "model tests"; PLINK's --model): out_path gets the header line
 *     #CHR POS ID A1 A2 AFF UNAFF CHISQ_GENO P_GENO CHISQ_TREND P_TREND CHISQ_ALLELIC P_ALLELIC CHISQ_DOM P_DOM CHISQ_REC P_REC
 * and one line per written variant, tab-separated, sorted by chromosome and position as hpgv_run_assoc's file: A1 is REF and A2 is
 * ALT as in the chi-square file, AFF is r0/r1/r2 and UNAFF is s0/s1/s2 (the genotype-class counts of the affected and the
 * unaffected cohort columns: hom-ref / het / hom-alt), and the five chi-squares and p-values are printed as
 * hpgv_host_format_f6 prints them (NaN for a zero margin).  Every batch goes through hpgv_assoc_model_text.
 *   n_perms == 0  writes that file only;
 *   n_perms >= 1  also writes <out_path>.mperm for the TREND statistic: header, line format, label generation
 *                 (hpgv_perm_labels_shuffle(seed)) and independence from batch_bytes, engine threads and devices are those of
 *                 hpgv_run_assoc_perm;
 *   n_perms < 0 or a NULL path: HPGV_ERR_INVALID before the engine is started, and no file is written.
 * Same cohort, filters, record filters and input forms (plain, gzip, bgzip) as hpgv_run_assoc. */
int  hpgv_run_assoc_model(const char *vcf_path, const char *ped_path, const char *out_path, int n_perms, uint64_t seed,
                          size_t batch_bytes, long *n_variants_out);
/* The association test with covariates (include/hpgv.h "Logistic regression"; PLINK's --logistic --covar, parity unpinned): one
 * logistic regression per variant of the phenotype on the ALT allele count and the covariates.  out_path gets the header line
 *     #CHR POS ID A1 A2 NOBS BETA SE OR STAT P ITER
 * and one line per written variant, tab-separated, sorted as hpgv_run_assoc_model's file.  A1 is REF and A2 is ALT as there; the
 * TESTED allele is ALT (PLINK tests the minor allele: a sign flip of BETA where ALT is the major one).  NOBS, ITER: n_obs and
 * iters of the row's hpgv_logistic_result; BETA, SE, STAT, P of the genotype coefficient and OR = exp(BETA), printed as
 * hpgv_host_format_f6 prints them; a failed fit (status not HPGV_LOGIT_OK) prints nan in the five.  Every batch goes through
 * hpgv_assoc_logistic_text with max_iter HPGV_RUN_LOGISTIC_MAX_ITER and tol HPGV_RUN_LOGISTIC_TOL; a row's result depends on
 * that row only, so the file does not depend on batch_bytes, engine threads, input form or devices.
 *   covar_path (may be NULL: no covariates): lines of whitespace-separated columns, two ids and then the values -- PLINK's
 *     --covar shape, and exactly what hpgv_run_pca writes as .eigenvec.  A first line whose first token is FID, #FID or #IID is a
 *     header.  The SECOND id is matched byte for byte against the VCF's sample names; lines of other samples are ignored.
 *   n_covar: the first n_covar value columns are used; 0 = all columns of the file.
 *   A cohort sample (PED PHENO 2 or 1) with no line, or with a value among the used columns that is not a finite number ("NA",
 *   "nan"), leaves the cohort: it becomes HPGV_COND_OTHER before hpgv_set_cohort.  *n_samples_used_out (may be NULL): the
 *   cohort samples that stayed.  The covariates are set on every device's context.
 * HPGV_ERR_INVALID before the engine is started, and no file written: a NULL path other than covar_path, n_covar < 0, n_covar > 0
 * without a file, a file that cannot be read, a line with fewer than two ids, a ragged line, a second id that appears twice, more
 * than HPGV_LOGISTIC_MAX_COVAR columns in use, n_covar above the file's columns.
 * Same cohort, filters, record filters and input forms (plain, gzip, bgzip) as hpgv_run_assoc_model. */
#define HPGV_RUN_LOGISTIC_MAX_ITER 25
#define HPGV_RUN_LOGISTIC_TOL 1e-10
int  hpgv_run_assoc_logistic(const char *vcf_path, const char *ped_path, const char *covar_path, int n_covar, const char *out_path,
                             size_t batch_bytes, long *n_variants_out, long *n_samples_used_out);
/* The association test of a quantitative trait with covariates (include/hpgv.h "Linear regression"; PLINK's --linear --covar,
 * parity unpinned): one ordinary least squares fit per variant of the trait on the ALT allele count and the covariates.  out_path
 * gets the header line
 *     #CHR POS ID A1 A2 NOBS BETA SE STAT P
 * and one line per written variant, tab-separated, sorted and formatted as hpgv_run_assoc_logistic's file; the tested allele is
 * ALT.  NOBS: n_obs of the row's hpgv_linear_result; BETA, SE, STAT (a signed t statistic), P of the genotype coefficient.  A
 * row with status HPGV_LINEAR_SINGULAR prints nan in the four, one with HPGV_LINEAR_EXACT its BETA, SE 0 and nan for STAT and P.
 * Every batch goes through hpgv_assoc_linear_text; a row's result depends on that row only, so the file does not depend on
 * batch_bytes, engine threads, input form or devices.
 *   pheno_path (PLINK's --pheno; may be NULL): a file of the covariate file's shape, whose first value column is the trait;
 *     ped_path may then be NULL.  Without it the trait is the PED's sixth column read as a number: a value that is not a
 *     finite number, or equals -9, is missing.
 *   covar_path, n_covar: as for hpgv_run_assoc_logistic.
 *   A sample enters the cohort (as HPGV_COND_UNAFFECTED: the condition only places a column) when it has a trait and, if
 *   covariates are used, a line of finite covariates; everyone else is HPGV_COND_OTHER.  *n_samples_used_out (may be NULL): the
 *   cohort's size.  The trait and the covariates are set on every device's context.  The inheritance record filters see no
 *   affected sample in this run.
 * HPGV_ERR_INVALID before the engine is started, and no file written: what hpgv_run_assoc_logistic refuses (ped_path may be NULL
 * here when pheno_path is not), both ped_path and pheno_path NULL, a phenotype file that cannot be read, is malformed as a
 * covariate file can be, or has no value column.
 * Same filters, record filters and input forms (plain, gzip, bgzip) as hpgv_run_assoc_logistic. */
int  hpgv_run_assoc_linear(const char *vcf_path, const char *ped_path, const char *pheno_path, const char *covar_path, int n_covar,
                           const char *out_path, size_t batch_bytes, long *n_variants_out, long *n_samples_used_out);
/* The same run with max(T) permutations of the linear statistic (include/hpgv.h "permutations of the linear statistic"; PLINK's
 * --linear --mperm): out_path is hpgv_run_assoc_linear's file byte for byte, and <out_path>.mperm holds "#CHR POS ID EMP1 EMP2" in
 * the format of the other permutation runs, nan where a row takes no part.  The orders are hpgv_perm_order_shuffle(seed) over the
 * cohort that stayed; every batch goes through hpgv_assoc_linear_perm_text (the records and the permutation in one call) and the
 * batches' maxima merge by maximum, so neither file depends on batch_bytes, engine threads, input form or devices.  A row with
 * missing calls is permuted with its mean-imputed dosage: its EMP1 / EMP2 belong to that statistic, not to the STAT column's fit
 * of the observed subset.  HPGV_ERR_INVALID before anything is opened for n_perms < 1 or a NULL path, and for what
 * hpgv_run_assoc_linear refuses; collinear covariates fail the run when the permutations are set. */
int  hpgv_run_assoc_linear_perm(const char *vcf_path, const char *ped_path, const char *pheno_path, const char *covar_path, int n_covar,
                                const char *out_path, int n_perms, uint64_t seed, size_t batch_bytes, long *n_variants_out,
                                long *n_samples_used_out);
/* The covariate file's reader on its own: the first n_covar value columns (0: all) for the samples names[0 .. n_names), cov with
 * HPGV_LOGISTIC_MAX_COVAR doubles per name, have[j] = 1 where names[j] has a line of finite values (else 0, and zeros in cov);
 * *n_covar_out: the columns used.  HPGV_ERR_INVALID as above (message in hpgv_host_last_error).  No GPU call. */
int  hpgv_host_covar_read(const char *covar_path, const char *const *names, int n_names, int n_covar, int *n_covar_out,
                          double *cov, uint8_t *have);
/* The stratified association test (include/hpgv.h "stratified association"; PLINK's --mh / --bd with --within, parity unpinned):
 * Cochran-Mantel-Haenszel, the Mantel-Haenszel odds ratio and Breslow-Day per variant over the strata of within_path.  out_path
 * gets the header line
 *     #CHR POS ID A1 A2 NSTRATA CHISQ_CMH P_CMH OR_MH SE L95 U95 CHISQ_BD P_BD
 * and one line per written variant, tab-separated, sorted as hpgv_run_assoc_model's file.  A1 is REF and A2 is ALT; NSTRATA is
 * n_strata_cmh of the row's hpgv_cmh_result, the numbers are its fields as hpgv_host_format_f6 prints them, nan for a NaN.  Every
 * batch goes through hpgv_assoc_cmh_text (rows on chromosome X by its rule); a row's result depends on that row only, so the file
 * does not depend on batch_bytes, engine threads, input form or devices.
 *   within_path: PLINK's --within shape, lines of two ids and a cluster name, whitespace-separated (further columns are ignored),
 *     with the header rule of the covariate file.  The SECOND id is matched byte for byte against the VCF's sample names; lines of
 *     other samples are ignored.  Strata are numbered by first appearance in VCF column order among the cohort samples.
 *   A cohort sample (PED PHENO 2 or 1) without a line becomes HPGV_COND_OTHER before hpgv_set_cohort, as a sample without
 *     covariates does in hpgv_run_assoc_logistic.  *n_samples_used_out (may be NULL): the cohort samples that stayed;
 *     *n_strata_out (may be NULL): their strata.  No cohort sample with a line: HPGV_ERR_INVALID.
 * HPGV_ERR_INVALID before the engine is started, and no file written: a NULL path, a within file that cannot be read, a line with
 * fewer than three columns, a ragged line, a second id that appears twice, more than HPGV_CMH_MAX_STRATA distinct cluster names in
 * the file.
 * Same cohort, filters, record filters and input forms (plain, gzip, bgzip) as hpgv_run_assoc_model. */
int  hpgv_run_assoc_cmh(const char *vcf_path, const char *ped_path, const char *within_path, const char *out_path,
                        size_t batch_bytes, long *n_variants_out, long *n_samples_used_out, int *n_strata_out);
/* The same run with max(T) label permutation within the strata (include/hpgv.h "Permutation within strata"; PLINK's --mh --mperm
 * with --within): out_path is hpgv_run_assoc_cmh's file byte for byte, and <out_path>.mperm holds "#CHR POS ID EMP1 EMP2" of
 * CHISQ_CMH in the format of the other permutation runs, nan where CHISQ_CMH is NaN.  The label rows are
 * hpgv_perm_labels_shuffle_within(seed) over the cohort that stayed and its strata; every batch goes through
 * hpgv_assoc_cmh_perm_text (the records and the permutation in one call) and the batches' maxima merge by maximum, so both files do
 * not depend on batch_bytes, engine threads, input form or devices.  n_perms < 1 is HPGV_ERR_INVALID before the engine starts, and
 * nothing is written; otherwise what hpgv_run_assoc_cmh refuses. */
int  hpgv_run_assoc_cmh_perm(const char *vcf_path, const char *ped_path, const char *within_path, const char *out_path,
                             int n_perms, uint64_t seed, size_t batch_bytes, long *n_variants_out, long *n_samples_used_out,
                             int *n_strata_out);
/* The within file's reader on its own: stratum[j] for the samples names[0 .. n_names) -- the number of the cluster on the line
 * whose second id is names[j], -1 without one or where take[j] (take may be NULL: everyone) is 0 -- clusters numbered by first
 * appearance in the order of names among the samples taken; *n_strata_out: how many.  HPGV_ERR_INVALID as above (message in
 * hpgv_host_last_error).  No GPU call. */
int  hpgv_host_within_read(const char *within_path, const char *const *names, int n_names, const uint8_t *take,
                           int32_t *stratum, int *n_strata_out);
/* hpgv_run_assoc with LD clumping of its results (PLINK's --clump, without overlap and without replication): out_path is
 * written byte for byte as hpgv_run_assoc writes it, and <out_path>.clumped beside it, which groups the significant variants
 * into clumps, each around its strongest variant.
 *   Candidates.  Every batch goes through hpgv_assoc_select_text with p_max = p2: the rows with p <= p2 are compacted on the
 *   device, and the writer stage appends the batch's candidate block and heads (CHR, POS, ID, p) to the run's store on the
 *   host, in batch order.  Only records the result file also writes are kept: one dropped only by a host-side field filter
 *   leaves the store there.  So the result depends neither on batch_bytes nor on the number of engine threads or devices.
 *   Edges.  At the end ONE hpgv_ld_edges call over the candidate store (on a group context: member 0) with the chromosomes
 *   numbered in order of first appearance, the positions, max_bp, min_r2, and `window` counted in CANDIDATES: a window of
 *   1 024 candidates spans about 100 000 variants of a genome-wide file.  Where the count exceeds the room the list grows and
 *   the call is repeated once.
 *   Clumps.  hpgv_clump(p of the candidates, the edges, p1), then the file: the header "#CHR\tPOS\tID\tP\tTOTAL\tSP2" and one
 *   line per clump in clump order (ascending p of the index variant, ties in file order): P printed with %.6e, TOTAL the
 *   number of claimed members, SP2 the members as CHR:POS joined by commas in file order, or NONE.
 *   *n_truncated_out (may be NULL) counts the candidates i for which candidate i + window + 1 exists, lies on the same
 *   chromosome and within max_bp (max_bp < 0: the distance condition is dropped): for those the candidate window cut the
 *   distance window short.  One WARN line on stderr when it is not 0.  *n_clumps_out (may be NULL): the clumps written.
 * HPGV_ERR_INVALID before the engine is started, and no file written: a NULL path or NULL options, p1 or p2 outside (0, 1],
 * p1 > p2, a NaN threshold, a window outside 1 .. HPGV_LD_MAX_WINDOW, a task other than CHI_SQUARE / FISHER.
 * Same cohort, filters, record filters and input forms (plain, gzip, bgzip) as hpgv_run_assoc. */
typedef struct { double p1, p2, min_r2; int64_t max_bp; int window; } hpgv_run_clump_options_t;
/* PLINK's defaults: 1e-4, 1e-2, 0.5, 250000; window HPGV_LD_MAX_WINDOW */
#define HPGV_RUN_CLUMP_DEFAULTS { 1e-4, 1e-2, 0.5, 250000, HPGV_LD_MAX_WINDOW }
int  hpgv_run_assoc_clump(const char *vcf_path, const char *ped_path, const char *out_path, enum ASSOC_task task,
                          const hpgv_run_clump_options_t *opt, size_t batch_bytes, long *n_variants_out,
                          long *n_clumps_out, long *n_truncated_out);
/* hpgv_run_tdt with max(T) family flips (include/hpgv.h "family flips"; PLINK's tdt --mperm): out_path is written byte for byte
 * as hpgv_run_tdt writes it, and <out_path>.mperm beside it with the header and line format of hpgv_run_assoc_perm's
 * ("#CHR\tPOS\tID\tEMP1\tEMP2", one line per written variant in the same sorted order, numbers as hpgv_host_format_f6 prints
 * them); NaN where the variant's chi-square is -1 (nothing transmitted).  The n_perms flip rows are generated once per run by
 * hpgv_perm_flips_shuffle(seed) over the PED's families (in order of first appearance, as hpgv_run_tdt builds them); every batch
 * goes through hpgv_tdt_perm_text and its maxima are merged into the run's by element-wise maximum, so the result depends
 * neither on batch_bytes nor on the number of engine threads or devices.  Same families, filters, record filters and input
 * forms (plain, gzip, bgzip) as hpgv_run_tdt.  n_perms < 1 or a NULL path: HPGV_ERR_INVALID before anything is opened. */
int  hpgv_run_tdt_perm(const char *vcf_path, const char *ped_path, const char *out_path, int n_perms, uint64_t seed,
                       size_t batch_bytes, long *n_variants_out);
/* record filters of the file-level runners (filter_records on every batch, assoc_runner.c:191; options
 * shared_options.c:42-47,86-115).  A negative member switches that filter off; NULL switches all off.  The
 * count-derived ones run on the GPU from the same tokenized batch:
 *   min_maf            --maf      keep records whose minor-allele frequency (first two alleles) is >= min_maf
 *   max_missing        --missing  keep records whose rate of missing genotypes is <= max_missing
 *   max_mendel_errors  --mendel   keep records with at most this many Mendelian errors over the PED's trios
 *   num_alleles        --alleles  keep records with exactly this many alleles (1 + ALT alleles)
 *   min_quality        --quality  keep records with QUAL >= min_quality
 * The filter bodies live in hpg-libs (absent from the reference tree): these are the definitions used here.
 * The setting applies to the runs started afterwards on this process. */
typedef struct {
    double min_maf, max_missing;
    int max_mendel_errors, num_alleles;
    double min_quality;
} hpgv_run_filters_t;
void hpgv_run_set_filters(const hpgv_run_filters_t *filters);
/* the rest of the reference's record filters (shared_options.c:42-56,86-173; --gene needs the CellBase web service and
 * is not here).  The filter bodies live in hpg-libs: these are the definitions used here.  Off as marked below.
 *   min_coverage   --coverage      keep records whose INFO has DP >= min_coverage (DP read as the split runner reads it:
 *                                  the first ';'-separated entry with the key DP; a record without DP, or with a bare DP
 *                                  flag, fails)
 *   regions        --region        keep records inside the regions: a comma-separated list of CHROM (the whole
 *                                  sequence), CHROM:POS or CHROM:START-END (1-based, inclusive, START <= END; the last
 *                                  ':' of an item separates CHROM, positions are decimal digits >= 1)
 *   region_file    --region-file   keep records inside the regions of a GFF file: tab-separated rows, blank and '#'
 *                                  lines skipped, column 1 the sequence, 3 the feature, 4 and 5 start and end (at least
 *                                  5 columns, start <= end)
 *   region_type    --region-type   with region_file: only the rows whose feature is exactly this (NULL: every row)
 *   snp            --snp           1 include: keep records whose ID is not "."; 0 exclude: keep those whose ID is "."
 *   var_type       --var-type      keep records of this type (HPGV_VAR_*):
 *                                    structural: some ALT allele is symbolic (begins with '<') or a breakend (holds
 *                                                '[' or ']');
 *                                    snv:        REF is one base and every ALT allele one base (the stats tool's SNP);
 *                                    indel:      not structural, and some ALT allele's length differs from REF's;
 *                                  an MNP, or ALT ".", is none of the three
 *   indel          --indel         1 include: keep what var_type HPGV_VAR_INDEL keeps; 0 exclude: keep every other record
 *   min_dominant   --inh-dom       keep records whose fraction of samples following a dominant / recessive inheritance
 *   min_recessive  --inh-rec       pattern is >= the threshold (definitions: hpgv.h hpgv_set_text_inheritance_filters;
 *                                  counted on the GPU).  Affected = PED PHENO 2, unaffected = PHENO 1 (vcf2epi: its own
 *                                  classes, every sample not affected being unaffected, dataset_creator.c:279-300);
 *                                  they need a PED: a runner started without one (aggregate always) returns
 *                                  HPGV_ERR_INVALID before the engine starts and writes no file
 * Regions match CHROM byte for byte; they are kept sorted and merged per sequence and looked up by binary search.  With
 * both regions and region_file set a record must fall in both.  A record whose POS is not a number (decimal digits)
 * fails a region filter.  The filters apply together with those of hpgv_run_set_filters in the assoc, tdt, aggregate,
 * filter and vcf2epi runners (stats and split ignore them).  The setter copies the strings and reads / parses the regions
 * when it is called; a malformed item or row, a file that cannot be read, a threshold above 1 or a value out of range
 * returns HPGV_ERR_INVALID (message in hpgv_host_last_error) and the previous setting stays in force.  NULL switches all
 * off.  The setting applies to the runs started afterwards on this process. */
enum { HPGV_VAR_SNV = 1, HPGV_VAR_INDEL = 2, HPGV_VAR_STRUCTURAL = 3 };
typedef struct {
    long min_coverage;                 /* --coverage     < 0 off */
    const char *regions;               /* --region       NULL off */
    const char *region_file;           /* --region-file  NULL off (GFF) */
    const char *region_type;           /* --region-type  NULL: every feature */
    int snp;                           /* --snp          -1 off, 0 exclude, 1 include */
    int var_type;                      /* --var-type     -1 off, HPGV_VAR_* */
    int indel;                         /* --indel        -1 off, 0 exclude, 1 include */
    double min_dominant, min_recessive;/* --inh-dom / --inh-rec  < 0 off, <= 1 */
} hpgv_run_record_filters_t;
int hpgv_run_set_record_filters(const hpgv_run_record_filters_t *f);

/* The form of what hpgv_run_filter and hpgv_run_split write (the other runners ignore it): HPGV_OUT_PLAIN, the default, is
 * text; with HPGV_OUT_BGZF the files are bgzip -- <out_prefix>.filtered.gz and <out_prefix>.rejected.gz, <out_dir>/<split
 * name>_<base>.gz -- that tabix, bcftools and these runners read: whole BGZF members of at most 65 280 text bytes and one
 * EOF block at the end of every file, the records deflated on the device that partitioned them.  What the files inflate to
 * is, byte for byte, what the plain run writes.  Without save_rejected the rejected records are neither deflated nor
 * copied, and .rejected.gz is the EOF block alone: a valid, empty bgzip file.  A run takes the setting as it is when it
 * starts.  An unknown mode returns HPGV_ERR_INVALID and the setting stays. */
enum { HPGV_OUT_PLAIN = 0, HPGV_OUT_BGZF = 1 };
int hpgv_run_set_output_compression(int mode);

/* run_filter (src/vcf-tools/filter/filter_runner.c:23-260, hpg-var-vcf filter): the records that pass the filters of
 * hpgv_run_set_filters to <out_prefix>.filtered, the others to <out_prefix>.rejected when save_rejected != 0 (--save-rejected,
 * main_filter.c:85; without it .rejected is created empty, filter_runner.c:63-68) -- with those of hpgv_run_set_record_filters
 * too.  Without any filter set (of either setter), or with NULL paths, or with --mendel, --inh-dom or --inh-rec and no PED,
 * it returns HPGV_ERR_INVALID before the engine starts and writes no file (the reference writes
 * nothing without a filter chain, hpg_variant_utils.c:220-226).  ped_path may be NULL; the count filters use every VCF column
 * (as hpgv_run_stats does), the Mendelian one the PED's trios whose three members are VCF columns.
 * Each file: the input header verbatim up to its #CHROM line, then one line per active filter, in this order and with the
 * thresholds printed by %g --
 *   ##FILTER=<ID=maf,Description="Minor allele frequency >= 0.1">
 *   ##FILTER=<ID=missing,Description="Rate of missing genotypes <= 0.1">
 *   ##FILTER=<ID=mendel,Description="Mendelian errors <= 1">
 *   ##FILTER=<ID=alleles,Description="Number of alleles == 2">
 *   ##FILTER=<ID=quality,Description="Quality >= 30">
 * and then, for hpgv_run_set_record_filters (the strings verbatim, '"' and '\' written \" and \\; region-file in its second
 * form with a region_type; snp / indel "exclude", var-type "indel" / "structural" as set) --
 *   ##FILTER=<ID=coverage,Description="Coverage >= 10">
 *   ##FILTER=<ID=region,Description="Regions 6:29000000-34000000">
 *   ##FILTER=<ID=region-file,Description="Regions of file genes.gff">
 *   ##FILTER=<ID=region-file,Description="Regions of file genes.gff of type exon">
 *   ##FILTER=<ID=snp,Description="SNP include">
 *   ##FILTER=<ID=var-type,Description="Variant type == snv">
 *   ##FILTER=<ID=indel,Description="Indels include">
 *   ##FILTER=<ID=inh-dom,Description="Samples following a dominant inheritance pattern >= 0.9">
 *   ##FILTER=<ID=inh-rec,Description="Samples following a recessive inheritance pattern >= 0.9">
 * -- then the #CHROM line as written, then the records byte for byte in file order (the reference writes its batches as its
 * workers finish them).  A last line without a newline gets one; a line with fewer than CHROM .. ALT is rejected; empty lines
 * go to neither file.  The lines of a batch are partitioned on the device that tokenized them (hpgv_text_partition), whatever
 * the input's compression.  *n_passed_out / *n_rejected_out (may be NULL): the records kept / rejected (counted with or
 * without save_rejected). */
int  hpgv_run_filter(const char *vcf_path, const char *ped_path, const char *out_prefix, int save_rejected,
                     size_t batch_bytes, long *n_passed_out, long *n_rejected_out);
/* run_split (src/vcf-tools/split/split_runner.c:23-190, split.c:37-122, hpg-var-vcf split): every record of the VCF to
 * <out_dir>/<split name>_<base>, <base> being the input's file name.  Split names (split_options_parsing.c:114-140):
 *   HPGV_SPLIT_CHROMOSOME   chromosome_<CHROM>
 *   HPGV_SPLIT_COVERAGE     by v = INFO's DP against the ascending bounds intervals[0 .. n_intervals - 1] = I0 < I1 < ...:
 *                           coverage_0_<I0> for v <= I0 (the low end is 0 whatever v), coverage_<Ij-1>_<Ij> for
 *                           Ij-1 < v <= Ij, coverage_<In-1>_N for v > In-1; numbers as %ld
 * Names are compared case-insensitively, as the reference's table of open files does (cp_hash_istring): chr1 and CHR1 go to
 * one file, named after the first such record in file order.  A file is created by its first record (a bucket without records
 * has no file) with the input header verbatim up to and including its #CHROM line, then holds its records byte for byte.
 * out_dir is created when missing (one level, as create_directory).  Where this differs from the reference on purpose:
 *   - records are written in file order within each file (the reference writes them as its workers finish);
 *   - a record whose INFO has no entry with the key exactly DP, or only a bare DP flag, goes to coverage_missing (the
 *     reference crashes in atoi(NULL)); entries are ';'-separated and the first DP counts; its value is read as atoi does --
 *     an optional sign, then digits up to the first non-digit, none giving 0 -- saturated at the int64 range;
 *   - a trailing .gz / .bgz is dropped from <base>: the files hold plain text by default; with
 *     hpgv_run_set_output_compression(HPGV_OUT_BGZF) they are bgzip and named <split name>_<base>.gz;
 *   - in file names only, '/' is written %2F and '%' is written %25, so no CHROM names a path outside out_dir;
 *   - lines with fewer than 8 fields (CHROM .. INFO), empty lines included, go to no file; a sites-only VCF is valid input;
 *   - a last line without a newline gets one;
 *   - at most 64 files are open at once (the reference keeps all open; a contig-rich assembly would run out of
 *     descriptors): the least recently written is closed and reopened later for appending.
 * NULL paths, an unknown criterion, coverage without intervals or with intervals that do not strictly increase, and an out_dir
 * that cannot be created return HPGV_ERR_INVALID before the engine starts, and no file is written.  The lines of a batch
 * are bucketed on the device that tokenized them (hpgv_text_multisplit), whatever the input's compression.
 * *n_records_out: records written; *n_files_out: files created; *n_skipped_out: lines that went to no file (each may be NULL). */
enum { HPGV_SPLIT_CHROMOSOME = 1, HPGV_SPLIT_COVERAGE = 2 };
int  hpgv_run_split(const char *vcf_path, const char *out_dir, int criterion, const long *intervals, int n_intervals,
                    size_t batch_bytes, long *n_records_out, long *n_files_out, long *n_skipped_out);
/* create_dataset_from_vcf (src/vcf-tools/vcf2epi/dataset_creator.c:24-222) without its filters: the binary
 * dataset hpgv_run_epistasis reads -- uint32 num_variants, num_affected, num_unaffected, then per variant
 * one byte per sample, cases first (0 "0/0", 1 heterozygous, 2 homozygous non-reference, 255 missing);
 * every sample that is not AFFECTED counts as unaffected (dataset_creator.c:279-300) */
int  hpgv_run_vcf2epi(const char *vcf_path, const char *ped_path, const char *out_path,
                      size_t batch_bytes, long *n_variants_out);
/* run_aggregate (src/vcf-tools/aggregate/aggregate_runner.c:23-222): the VCF without its samples, every record's
 * INFO extended by HPG_AC, HPG_AF, HPG_AN (AC / AF / AN replacing the record's own with overwrite != 0) and HPG_GTC,
 * computed by get_variants_stats on the GPU.  Values as merge_info_and_stats (:262-365) and
 * report_variant_genotypes_stats (:376-403) print them; the order of the INFO fields is original fields first, then
 * AC, AF, AN, GTC (the reference walks a hash table); QUAL is copied as written. */
int  hpgv_run_aggregate(const char *vcf_path, const char *out_path, int overwrite, size_t batch_bytes,
                        long *n_variants_out);
/* run_stats (src/vcf-tools/stats/stats_runner.c:23-420): <out_prefix>.stats-variants / .stats-samples /
 * .stats-summary from one pass over the VCF; with a PED also the Mendelian errors and one
 * <out_prefix>.phenotype-<value>.stats-variants per value of its phenotype column (stats_runner.c:267-297); ped_path
 * may be NULL.  The report
 * writers of the reference live in hpg-libs; the three files are tab-separated renderings of the same fields
 * (header lines name the columns). */
int  hpgv_run_stats(const char *vcf_path, const char *ped_path, const char *out_prefix, size_t batch_bytes,
                    long *n_variants_out);
/* Sample relatedness (include/hpgv.h "IBS"; PLINK's --genome, parity unpinned): duplicates, undeclared relatives, sample swaps.
 * Every batch goes through hpgv_ibs_text into one buffer of pair counts per device of the run (the kernel's atomics make the
 * engine threads safe; the devices' buffers are added when the run ends: integers, any order).  The lines hpgv_run_assoc would
 * not count -- not a record -- and the lines on chromosome "X" take no part.  The writer stage adds hpgv_ibs_terms of the
 * records' class counts in file order, so E, and with it the file, does not depend on batch_bytes, engine threads or devices.
 * As in hpgv_run_stats, the filters of hpgv_run_set_filters and hpgv_run_set_record_filters are not applied.  When the input is
 * read, hpgv_ibs_select_dev gives the pairs with PI_HAT >= min_pi_hat (a NaN PI_HAT never qualifies; the call is repeated once
 * with room when the list was too short), and out_path gets the header line
 *     #IID1 IID2 NM IBS0 IBS1 IBS2 Z0 Z1 Z2 PI_HAT DST
 * and one line per pair, tab-separated, sorted by (column of IID1, column of IID2): the sample names of the #CHROM line, the four
 * counts, and hpgv_ibs_genome's five values as hpgv_host_format_f6 prints them.  *n_variants_out: the records that took part;
 * *n_pairs_out: the pairs written.  Input forms (plain, gzip, bgzip) as hpgv_run_assoc.  A NULL path or a NaN min_pi_hat:
 * HPGV_ERR_INVALID before anything is opened, and no file is written.  The counts take 16 n_samples^2 bytes of device memory. */
int  hpgv_run_genome(const char *vcf_path, const char *out_path, double min_pi_hat, size_t batch_bytes,
                     long *n_variants_out, long *n_pairs_out);
/* The genetic relationship matrix of the VCF's samples (include/hpgv.h "GRM"; GCTA's --make-grm-bin, parity unpinned) at
 * frac_bits = hpgv_grm_frac_bits(min_maf).  Every batch goes through hpgv_grm_text into one buffer of pair sums per device of
 * the run, 16 n_samples^2 bytes each, dealt as hpgv_run_genome deals them; the devices' buffers are added as integers when the
 * run ends.  Lines that are not records and lines on chromosome "X" take no part; as in hpgv_run_genome neither filter setter is
 * applied.  The sums are integers, so the three files do not depend on batch_bytes, engine threads, input form or devices:
 *     <out_prefix>.grm.bin     float32 of hpgv_grm_value, rows i = 0 .. n - 1, columns j = 0 .. i (native byte order)
 *     <out_prefix>.grm.N.bin   float32 of the pair's n, in the same order
 *     <out_prefix>.grm.id      "name<TAB>name" per sample of the #CHROM line
 * *n_variants_out: the USED records (not X, 0 < Y < T, MAF >= min_maf); *n_samples_out: n.  Input forms as hpgv_run_assoc.  A
 * NULL path or a min_maf outside (0, 0.5] (NaN included): HPGV_ERR_INVALID before anything is opened, and no file is written. */
int  hpgv_run_grm(const char *vcf_path, const char *out_prefix, double min_maf, size_t batch_bytes,
                  long *n_variants_out, long *n_samples_out);
/* The first n_pcs principal components of that matrix (include/hpgv.h "PCA"; GCTA's and PLINK's --pca, parity unpinned).  The
 * pass over the VCF is hpgv_run_grm's, unchanged; then the integer sum of the devices' buffers goes to the first device,
 * hpgv_grm_matrix_dev makes the f64 matrix there and hpgv_pca_dev solves it with tol = HPGV_RUN_PCA_TOL, max_iter =
 * HPGV_RUN_PCA_MAX_ITER and seed = HPGV_RUN_PCA_SEED.  The sums are integers and the solver is deterministic, so the files do not
 * depend on batch_bytes, engine threads, input form or devices:
 *     <out_prefix>.eigenval    one "%.8g" value per line, decreasing
 *     <out_prefix>.eigenvec    per sample "name<TAB>name" and n_pcs values in "%.8g", tab-separated
 * and, with write_grm != 0, hpgv_run_grm's three files, byte for byte.  *n_iter_out: the sweeps done.  A run that does NOT
 * converge within max_iter (a cohort without structure: include/hpgv.h "PCA") still writes the files, with the last Ritz pairs,
 * and returns HPGV_OK; it says so by *n_iter_out = -max_iter.  No file at all is written by: a pair of samples with n = 0 (a
 * sample without calls: drop it) -- HPGV_ERR_UNSUPPORTED; n_pcs outside [1, 24] or above the sample count, a NULL path, a bad
 * min_maf -- HPGV_ERR_INVALID. */
#define HPGV_RUN_PCA_TOL 1e-8
#define HPGV_RUN_PCA_MAX_ITER 1000
#define HPGV_RUN_PCA_SEED 1ull
int  hpgv_run_pca(const char *vcf_path, const char *out_prefix, double min_maf, int n_pcs, int write_grm, size_t batch_bytes,
                  long *n_variants_out, long *n_samples_out, int *n_iter_out);
/* The same solver on <grm_prefix>.grm.bin and .grm.id of an earlier run (as gcta --grm X --pca): the float32 lower triangle
 * widened to f64 and mirrored, the lines of .grm.id copied in front of the vectors.  Files, constants and *n_iter_out as
 * hpgv_run_pca.  A NaN element (a pair with n = 0): HPGV_ERR_UNSUPPORTED; a NULL path, unreadable files, sizes that do not
 * agree, n_pcs outside [1, 24] or above the sample count: HPGV_ERR_INVALID; no file is written by any of them. */
int  hpgv_run_pca_grm(const char *grm_prefix, const char *out_prefix, int n_pcs, long *n_samples_out, int *n_iter_out);
/* Allele scoring (include/hpgv.h "Score"; PLINK's --score, parity unpinned): per sample the sums of per-variant weights times ALT
 * counts -- polygenic scores, the projection of a cohort onto SNP loadings, burden counts.
 *   score_path: lines of whitespace-separated columns: a variant ID, an allele, then 1 .. 32 weight columns, the same number on
 *     every line.  A first line whose first token is ID, #ID or SNP is a header and names the score columns; otherwise they are
 *     SCORE1, SCORE2, ...  Column k is scored at frac_bits hpgv_score_frac_bits(max |w| of the column over the file): known before
 *     the pass, so every batch uses the same scale.
 *   A record takes part when its ID is in the file and the file's allele equals its ALT byte for byte, or equals its REF -- the
 *     weight then counts REF alleles (HPGV_SCORE_FLIP).  Skipped: a record whose ALT holds a ',', whose ID is "." or is not in the
 *     file, on chromosome X (hpgv_score_text's rule); and one whose allele is neither REF nor ALT, which is also counted in
 *     *n_unmatched_out (wherever it lies).  impute != 0: PLINK's default mean imputation; 0: no-mean-imputation.
 *   out_path: the header "#FID IID CNT CNT2" and "<name>_SUM <name>_AVG" per score, then one line per sample of the #CHROM line, in
 *     VCF order, tab-separated: FID = IID = the sample name (as .grm.id), CNT = 2 (impute ? n_used : n_called), CNT2 = n_alt,
 *     the values in "%.8g" (nan for 0 / 0) as .eigenvec's -- a projection goes straight into hpgv_run_assoc_logistic's covar_path,
 *     whose reader takes the header by its #FID rule.
 * *n_variants_out: the USED records (n_used), *n_samples_out: the samples.  Every sum is an integer, added over batches, engine
 * threads and devices (the devices' buffers on the host when the run ends), so the file does not depend on batch_bytes, engine
 * threads, input form or devices.  Neither filter setter is applied, as in hpgv_run_grm; input forms as hpgv_run_assoc.
 * HPGV_ERR_INVALID before the engine is started, and no file written: a NULL path, a score file that cannot be read or holds no
 * line of weights, a line with fewer than three columns, a ragged line, a weight that is not a finite number, an ID that appears twice, more
 * than 32 weight columns. */
int  hpgv_run_score(const char *vcf_path, const char *score_path, const char *out_path, int impute, size_t batch_bytes,
                    long *n_variants_out, long *n_samples_out, long *n_unmatched_out);
/* stage times of the last run on this process: {read, engine, write, sort, total} seconds and the number of
 * batches; read / engine / write overlap (three threads, three batch buffers in rotation).  The reader and
 * formatter teams use HPGV_IO_THREADS threads (environment; default half the cores, at most 16);
 * HPGV_RUN_TRACE=1 prints the same numbers to stderr. */
void hpgv_host_last_run_times(double *seconds6);

/* ---- epistasis (hpg-var-gwas epi): k-fold cross-validation helpers and the run over a vcf2epi dataset ------ */
/* cross_validation.c:16-100 and :247-281, same signatures; the shuffle uses rand() */
int **get_k_folds(unsigned int num_samples_affected, unsigned int num_samples_unaffected, unsigned int k,
                  unsigned int **sizes);
uint8_t *get_k_folds_masks(unsigned int num_samples_affected, unsigned int num_samples_unaffected, unsigned int k,
                           int **folds, unsigned int *sizes);
/* run_epistasis (singlenode/epistasis_runner.c:23-330) for pairs of SNPs: dataset file in, one report
 * <out_prefix>.cv<r>.epi per repetition out (epistasis_report.c:30-81).  eval_subset HPGV_EPI_TESTING /
 * HPGV_EPI_TRAINING; eval_mode 0 = CV-c (consistency), 1 = CV-a (accuracy). */
int  hpgv_run_epistasis(const char *dataset_path, int num_folds, int num_cv_repetitions, int max_ranking_size,
                        int eval_subset, int eval_mode, const char *out_prefix);
/* the same for combinations of `order` SNPs (the --order option, main_epistasis.c:128,142): 2 and 3 through the tile scans,
 * 4 and 5 through the listed-combination kernel (hpgv.h "ANY order"); report lines as epistasis_report.c:62-77 writes them
 * for any order: "( i, j, k, l )" and risky cells "(a-b, c, d), " */
int  hpgv_run_epistasis_order(const char *dataset_path, int order, int num_folds, int num_cv_repetitions,
                              int max_ranking_size, int eval_subset, int eval_mode, const char *out_prefix);

/* The runners' reader on its own: copies `in_path` (plain / gzip / BGZF) to `out_path` in the whole-line
 * batches (at most batch_bytes each) the runners hand to the engine, optionally after consuming the VCF
 * header as the runners do; *n_batches may be NULL. */
int  hpgv_host_copy_lines(const char *in_path, const char *out_path, size_t batch_bytes, int skip_vcf_header,
                          long *n_batches);

/* ---- staging (GT text -> HPGV8), exposed for tests ---------------------------- */
int  get_field_position_in_format(const char *field, char *format);
int  get_alleles(char *sample, int genotype_position, int *allele1, int *allele2);
/* out: num_variants x num_samples bytes, row-major; is_x: num_variants flags.  A caller that is alone (not inside an
 * OpenMP parallel region) has its batch's records dealt to HPGV_STAGE_THREADS workers (environment; default 8, at
 * most the cores; 1 = never); inside the runner's own worker team the caller stages its batch itself. */
int  hpgv_host_stage_records(vcf_record_t **variants, int num_variants, int num_samples,
                             int strict, uint8_t *out, uint8_t *is_x);

/* ---- where a per-batch adapter call spends its time (tools/bench_adapter.c) ---------------------------------
 * hpgv_host_adapter_profile(1) switches the clocks on (four clock_gettime per call); hpgv_host_adapter_times
 * returns what assoc_test / tdt_test / get_variants_stats calls have accumulated since the last reset, summed over
 * the calling threads: seconds4 = {staging (sample strings -> bytes), engine (cohort check + the hpgv_* call),
 * records (result structs, strings, list inserts), whole call}; *calls (may be NULL) their number. */
void hpgv_host_set_stage_threads(int n);        /* the team of a lone caller's staging; 0 = back to HPGV_STAGE_THREADS / default */
void hpgv_host_adapter_profile(int on);
void hpgv_host_adapter_times(double *seconds4, long *calls, int reset);

/* ---- Environment ----------------------------------------------------------------------------------------------
 * libhpgv_host.so reads the environment when the engine is bound (the first adapter / runner call, or hpgv_host_init*)
 * and at the start of every file run (hpgv_run_*, hpgv_host_copy_lines) -- never per batch, per block or per launch.
 *   HPGV_DEVICES=0,1,2,3 | all   devices of the engine when no hpgv_host_init* call named them (default: device 0)
 *   HPGV_IO_THREADS=n            reader / formatter team of a run (default: half the cores, at most 16)
 *   HPGV_STAGE_THREADS=n         team a lone adapter caller's staging is dealt to (default 8; 1 = never)
 *   HPGV_ENGINE_THREADS=n        batches in flight on the devices (default: by the input)
 *   HPGV_RUN_TRACE=1             stage times of a run on stderr
 *   HPGV_BGZF_VERIFY=0           no CRC-32 check of decoded BGZF blocks (default 1: checked, on the device where decoded there)
 *   HPGV_NO_GPU_INFLATE=1        bgzip decoded on the host          HPGV_ZLIB_INFLATE=1     ... through zlib
 *   HPGV_BGZF_ONE_DEVICE=1       a group decodes a bgzip file on its first device only (default: in parts, one per device)
 *   HPGV_NO_NUMA_BIND=1          a run's threads are not moved to the GPU's NUMA node
 *   HPGV_ALWAYS_SORT=1           the output file is sorted even when it came out in order
 *   HPGV_DECODE_TILES=0          the device's CRC check leaves no tokenizer tile records (windows of decoded text are then
 *                                tokenized with their counting sweep: the A/B of that short cut)
 * Diagnosis and tests (each switches one stage of the bgzip device path to its fall-back): HPGV_NO_DEVICE_WINDOWS,
 * HPGV_NO_LARGE_WINDOWS, HPGV_BGZF_HOST_TABLE, HPGV_SERIAL_BGZF_WALK, HPGV_NO_GROWING_TEXT, HPGV_NO_LOW_PRIORITY,
 * HPGV_NO_WRITER_THREAD, HPGV_UPLOAD_SEGMENT_MB, HPGV_UPLOAD_INFLIGHT, HPGV_TEST_GPU_INFLATE_REFUSE_EVERY,
 * HPGV_TEST_GPU_INFLATE_DAMAGE_EVERY (every n-th block's text is overwritten on the device between the decoder and the CRC
 * check: the check must catch it and the host's patch put it right), HPGV_TEST_SCAN_ROWS (no stretch of the stager longer than this many blocks, whether its rows come from the device's scan
 * or from the host's table), HPGV_TEST_TEXT_ESTIMATE_PERCENT, HPGV_BGZF_PART_MIN_KB (host/hpgv_host_internal.h: host_env_t).
 * The engine underneath has its own short table: include/hpgv.h "Environment". */

#ifdef __cplusplus
}
#endif
#endif
