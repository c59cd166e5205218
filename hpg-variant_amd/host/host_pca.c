/* host_pca.c -- the principal components of a run's relationship matrix (include/hpgv.h "PCA"): the end of a GRM run that asks
 * for them (hpgv_run_pca: the devices' sums on the first device, hpgv_grm_matrix_dev, hpgv_pca_dev, <prefix>.eigenval and
 * .eigenvec), and the same solver on the .grm.bin / .grm.id files of an earlier run (hpgv_run_pca_grm).
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"
#include <math.h>

/* the solver on a device matrix and the two files: ids[j] is the "fam<TAB>id" head of sample j's line.  *n_iter_out: the sweeps,
 * negated when the run did not converge */
static int pca_solve_write(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, int k, char **ids, const char *out_prefix, int *n_iter_out) {
    double *val = (double *)malloc(sizeof(double) * (size_t)k), *res = (double *)malloc(sizeof(double) * (size_t)k);
    double *vec = (double *)malloc(sizeof(double) * (size_t)k * (size_t)n);
    int rc = val && res && vec ? HPGV_OK : HPGV_ERR_NOMEM, n_iter = 0, converged = 0;
    if (!rc && (rc = hpgv_pca_dev(ctx, d_A, n, lda, k, HPGV_RUN_PCA_TOL, HPGV_RUN_PCA_MAX_ITER, HPGV_RUN_PCA_SEED, val, vec, res, &n_iter, &converged)))
        snprintf(g_err, sizeof g_err, "hpgv_pca_dev failed (%d): %s", rc, hpgv_last_error(ctx));
    char *text = NULL;
    size_t len = 0, cap = 0;
    if (!rc) {
        cap = (size_t)k * 32 + 1;
        if (!(text = (char *)malloc(cap))) rc = HPGV_ERR_NOMEM;
        for (int c = 0; c < k && !rc; c++) len += (size_t)sprintf(text + len, "%.8g\n", val[c]);
        if (!rc) rc = grm_put(out_prefix, ".eigenval", text, len);
        free(text); text = NULL; len = 0;
    }
    if (!rc) {
        for (int j = 0; j < n; j++) cap += strlen(ids[j]) + (size_t)k * 32 + 2;
        if (!(text = (char *)malloc(cap))) rc = HPGV_ERR_NOMEM;
        for (int j = 0; j < n && !rc; j++) {
            len += (size_t)sprintf(text + len, "%s", ids[j]);
            for (int c = 0; c < k; c++) len += (size_t)sprintf(text + len, "\t%.8g", vec[(size_t)j * (size_t)k + (size_t)c]);
            text[len++] = '\n';
        }
        if (!rc) rc = grm_put(out_prefix, ".eigenvec", text, len);
        free(text);
    }
    if (!rc && n_iter_out) *n_iter_out = converged ? n_iter : -n_iter;
    free(val); free(res); free(vec);
    return rc;
}

static size_t pca_pitch(int n) { return ((size_t)n + 1) & ~(size_t)1; }

int run_pca_write(run_t *R, const char *out_prefix) {
    run_genome_t *G = R->GN;
    const int n = R->n_samples;
    if (R->n_pcs > n) { snprintf(g_err, sizeof g_err, "n_pcs %d: the file has %d samples", R->n_pcs, n); return HPGV_ERR_INVALID; }
    hpgv_ctx *ctx = G->ctx[0];
    hpgv_grm_acc *sum = NULL;
    int rc = run_grm_sum(R, &sum);
    const size_t lda = pca_pitch(n), recs = (size_t)n * (size_t)n;
    void *d_A = NULL, *d_empty = NULL;
    uint64_t n_empty = 0;
    if (!rc && G->n_dev > 1 && (rc = hpgv_memcpy_h2d(ctx, G->d_counts[0], sum, recs * sizeof *sum, NULL))) host_fail("hpgv_memcpy_h2d", rc);
    if (!rc && (rc = hpgv_dev_alloc(ctx, lda * (size_t)n * sizeof(double), &d_A))) host_fail("hpgv_dev_alloc", rc);
    if (!rc && (rc = hpgv_dev_alloc(ctx, 16, &d_empty))) host_fail("hpgv_dev_alloc", rc);
    if (!rc && ((rc = hpgv_grm_matrix_dev(ctx, (const hpgv_grm_acc *)G->d_counts[0], n, R->frac_bits, (double *)d_A, lda, (uint64_t *)d_empty, NULL)) ||
                (rc = hpgv_memcpy_d2h(ctx, &n_empty, d_empty, sizeof n_empty, NULL))))
        snprintf(g_err, sizeof g_err, "hpgv_grm_matrix_dev failed (%d): %s", rc, hpgv_last_error(ctx));
    if (!rc && n_empty) {
        snprintf(g_err, sizeof g_err, "%llu pairs of samples share no used variant (a sample without calls?): drop the sample, the matrix has no value there",
                 (unsigned long long)n_empty);
        rc = HPGV_ERR_UNSUPPORTED;
    }
    if (!rc) {
        char **ids = (char **)malloc(sizeof *ids * (size_t)n);
        if (!ids) rc = HPGV_ERR_NOMEM;
        for (int j = 0; j < n && !rc; j++) {
            const size_t l = strlen(R->names[j]);
            if (!(ids[j] = (char *)malloc(2 * l + 2))) { for (int q = 0; q < j; q++) free(ids[q]); rc = HPGV_ERR_NOMEM; break; }
            sprintf(ids[j], "%s\t%s", R->names[j], R->names[j]);
        }
        if (!rc) {
            rc = pca_solve_write(ctx, (const double *)d_A, n, lda, R->n_pcs, ids, out_prefix, &R->n_iter);
            for (int j = 0; j < n; j++) free(ids[j]);
        }
        free(ids);
    }
    if (!rc && R->write_grm) rc = run_grm_files(R, out_prefix, sum);
    if (d_A) (void)hpgv_dev_free(ctx, d_A);
    if (d_empty) (void)hpgv_dev_free(ctx, d_empty);
    free(sum);
    return rc;
}

/* a whole file in memory (a NUL after it); NULL when it cannot be read */
static char *pca_slurp(const char *prefix, const char *suffix, size_t *bytes) {
    char *path = (char *)malloc(strlen(prefix) + strlen(suffix) + 1), *buf = NULL;
    if (!path) return NULL;
    strcpy(path, prefix); strcat(path, suffix);
    FILE *f = fopen(path, "rb");
    long size = -1;
    if (f && fseek(f, 0, SEEK_END) == 0 && (size = ftell(f)) >= 0 && fseek(f, 0, SEEK_SET) == 0 && (buf = (char *)malloc((size_t)size + 1))) {
        if (fread(buf, 1, (size_t)size, f) != (size_t)size) { free(buf); buf = NULL; }
        else { buf[size] = 0; *bytes = (size_t)size; }
    }
    if (f) fclose(f);
    if (!buf) snprintf(g_err, sizeof g_err, "cannot read %s", path);
    free(path);
    return buf;
}

int hpgv_run_pca_grm(const char *grm_prefix, const char *out_prefix, int n_pcs, long *n_samples_out, int *n_iter_out) {
    if (n_samples_out) *n_samples_out = 0;
    if (n_iter_out) *n_iter_out = 0;
    if (!grm_prefix || !out_prefix) { snprintf(g_err, sizeof g_err, "grm_prefix and out_prefix must not be NULL"); return HPGV_ERR_INVALID; }
    if (n_pcs < 1 || n_pcs > 24) { snprintf(g_err, sizeof g_err, "n_pcs %d: 1 .. 24", n_pcs); return HPGV_ERR_INVALID; }
    size_t id_bytes = 0, bin_bytes = 0;
    char *idtext = pca_slurp(grm_prefix, ".grm.id", &id_bytes), *bin = idtext ? pca_slurp(grm_prefix, ".grm.bin", &bin_bytes) : NULL;
    if (!idtext || !bin) { free(idtext); free(bin); return HPGV_ERR_INVALID; }
    int rc = HPGV_OK;
    size_t n = 0;
    for (size_t k = 0; k < id_bytes; k++) n += idtext[k] == '\n';
    if (id_bytes && idtext[id_bytes - 1] != '\n') n++;
    char **ids = (char **)malloc(sizeof *ids * (n ? n : 1));
    double *A = NULL;
    const size_t lda = pca_pitch((int)n);
    if (!ids) rc = HPGV_ERR_NOMEM;
    else if (n > 0x7FFFFFFFu || bin_bytes != n * (n + 1) / 2 * sizeof(float)) {
        snprintf(g_err, sizeof g_err, "%s.grm.bin holds %zu bytes, the %zu samples of .grm.id need %zu", grm_prefix, bin_bytes, n, n * (n + 1) / 2 * sizeof(float));
        rc = HPGV_ERR_INVALID;
    } else if ((size_t)n_pcs > n) { snprintf(g_err, sizeof g_err, "n_pcs %d: the matrix has %zu samples", n_pcs, n); rc = HPGV_ERR_INVALID; }
    if (!rc) {
        char *p = idtext;
        for (size_t j = 0; j < n; j++) {                  /* the lines in place: "fam<TAB>id" */
            ids[j] = p;
            char *e = strchr(p, '\n');
            if (e) { *e = 0; if (e > p && e[-1] == '\r') e[-1] = 0; p = e + 1; }
        }
        if (!(A = (double *)calloc(lda * n, sizeof *A))) rc = HPGV_ERR_NOMEM;
    }
    if (!rc) {                                            /* the float32 lower triangle widened and mirrored */
        const float *v = (const float *)bin;
        size_t at = 0;
        for (size_t i = 0; i < n && !rc; i++)
            for (size_t j = 0; j <= i; j++, at++) {
                if (v[at] != v[at]) { snprintf(g_err, sizeof g_err, "%s.grm.bin: NaN at (%zu, %zu): a pair without a shared variant; drop the sample", grm_prefix, i, j); rc = HPGV_ERR_UNSUPPORTED; break; }
                A[i * lda + j] = A[j * lda + i] = (double)v[at];
            }
    }
    void *d_A = NULL;
    if (!rc) rc = ensure_engine();
    hpgv_ctx *ctx = NULL;
    if (!rc) {
        ctx = hpgv_group_size(g_ctx) > 1 ? hpgv_group_member(g_ctx, 0) : g_ctx;
        if ((rc = hpgv_dev_alloc(ctx, lda * n * sizeof(double), &d_A))) host_fail("hpgv_dev_alloc", rc);
    }
    if (!rc && (rc = hpgv_memcpy_h2d(ctx, d_A, A, lda * n * sizeof(double), NULL))) host_fail("hpgv_memcpy_h2d", rc);
    if (!rc) rc = pca_solve_write(ctx, (const double *)d_A, (int)n, lda, n_pcs, ids, out_prefix, n_iter_out);
    if (!rc && n_samples_out) *n_samples_out = (long)n;
    if (d_A) (void)hpgv_dev_free(ctx, d_A);
    free(A); free(ids); free(idtext); free(bin);
    return rc;
}
