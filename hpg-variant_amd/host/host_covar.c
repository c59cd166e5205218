/* host_covar.c -- the covariate file of hpgv_run_assoc_logistic (include/hpgv_host.h): whitespace-separated lines of two id columns
 * and the values, the shape of PLINK's --covar and of the .eigenvec file hpgv_run_pca writes.  Read whole before the engine
 * starts (covar_table_read), matched to the VCF's sample names afterwards (covar_table_match).
 * The within file of hpgv_run_assoc_cmh (PLINK's --within: two ids and a cluster name) goes through the same reader: within_table_read,
 * within_table_match.
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"
#include <ctype.h>

void covar_table_free(covar_table_t *T) {
    if (!T) return;
    free(T->iid); free(T->c1); free(T->val); free(T->blob);
    memset(T, 0, sizeof *T);
}

static int is_header_token(const char *t, size_t n) {
    return (n == 3 && !memcmp(t, "FID", 3)) || (n == 4 && (!memcmp(t, "#FID", 4) || !memcmp(t, "#IID", 4)));
}

/* a value column's text: a finite number, or NaN for anything else ("NA", "nan", "inf", a stray word) */
static double covar_value(const char *t, size_t n) {
    char buf[64];
    if (n == 0 || n >= sizeof buf) return NAN;
    memcpy(buf, t, n); buf[n] = 0;
    char *end = NULL;
    const double v = strtod(buf, &end);
    return end == buf + n && isfinite(v) ? v : NAN;
}

static int cmp_iid(const void *a, const void *b) { return strcmp(*(char *const *)a, *(char *const *)b); }

/* the file's lines: T->n of them, T->ncols value columns each (every column of the file), iid[i] the second id, val[i * ncols + k]
 * NaN where the text is not a finite number, c1[i] the text of the first value column (NULL without one).  HPGV_ERR_INVALID with
 * the message in g_err: unreadable file, a line with fewer than two ids, a ragged line, a duplicate second id.  what: the file's
 * name in the messages ("covariate", "within") */
static int table_read(const char *path, covar_table_t *T, const char *what) {
    memset(T, 0, sizeof *T);
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(g_err, sizeof g_err, "cannot open the %s file %s", what, path); return HPGV_ERR_INVALID; }
    size_t len = 0, cap = 1 << 16;
    char *blob = (char *)malloc(cap + 1);
    for (size_t got; blob && (got = fread(blob + len, 1, cap - len, f)) > 0;) {
        len += got;
        if (len == cap) { cap *= 2; char *nb = (char *)realloc(blob, cap + 1); if (!nb) { free(blob); blob = NULL; } else blob = nb; }
    }
    const int bad_read = ferror(f);
    fclose(f);
    if (!blob) return HPGV_ERR_NOMEM;
    if (bad_read) { free(blob); snprintf(g_err, sizeof g_err, "cannot read the %s file %s", what, path); return HPGV_ERR_INVALID; }
    blob[len] = 0;
    T->blob = blob;
    size_t n_lines = 1;
    for (size_t i = 0; i < len; i++) if (blob[i] == '\n') n_lines++;
    T->iid = (char **)malloc(sizeof(char *) * n_lines);
    T->c1 = (char **)malloc(sizeof(char *) * n_lines);
    if (!T->iid || !T->c1) { covar_table_free(T); return HPGV_ERR_NOMEM; }
    int rc = HPGV_OK, first = 1;
    long line_no = 0;
    size_t val_cap = 0;
    for (char *l = blob; rc == HPGV_OK && l < blob + len;) {
        char *e = memchr(l, '\n', (size_t)(blob + len - l));
        if (!e) e = blob + len;
        char *next = e < blob + len ? e + 1 : e;
        line_no++;
        /* the tokens of [l, e) */
        int ntok = 0, cols = 0;
        char *iid = NULL, *c1 = NULL; size_t iid_len = 0, c1_len = 0;
        int header = 0;
        for (char *p = l; p < e;) {
            while (p < e && isspace((unsigned char)*p)) p++;
            if (p >= e) break;
            char *t = p;
            while (p < e && !isspace((unsigned char)*p)) p++;
            const size_t tn = (size_t)(p - t);
            if (ntok == 0 && first && is_header_token(t, tn)) { header = 1; break; }
            if (ntok == 1) { iid = t; iid_len = tn; }
            if (ntok == 2) { c1 = t; c1_len = tn; }
            if (ntok >= 2) {
                if (T->ncols_set && cols >= T->ncols) { cols++; ntok++; continue; }      /* (ragged: found below) */
                if ((size_t)T->n * (size_t)(T->ncols_set ? T->ncols : 0) + (size_t)cols >= val_cap) {
                    val_cap = val_cap ? 2 * val_cap : 1024;
                    double *nv = (double *)realloc(T->val, sizeof(double) * val_cap);
                    if (!nv) { rc = HPGV_ERR_NOMEM; break; }
                    T->val = nv;
                }
                T->val[(size_t)T->n * (size_t)(T->ncols_set ? T->ncols : 0) + (size_t)cols] = covar_value(t, tn);
                cols++;
            }
            ntok++;
        }
        if (rc) break;
        if (header) { first = 0; l = next; continue; }
        if (ntok == 0) { l = next; continue; }                        /* an empty line */
        first = 0;
        if (ntok < 2) { snprintf(g_err, sizeof g_err, "%s line %ld: fewer than two id columns", path, line_no); rc = HPGV_ERR_INVALID; break; }
        if (!T->ncols_set) { T->ncols = cols; T->ncols_set = 1; }
        else if (cols != T->ncols) { snprintf(g_err, sizeof g_err, "%s line %ld: %d value columns, the lines before it have %d", path, line_no, cols, T->ncols); rc = HPGV_ERR_INVALID; break; }
        iid[iid_len] = 0;                                             /* (the separator behind it, or the blob's own NUL) */
        if (c1) c1[c1_len] = 0;
        T->c1[T->n] = c1;
        T->iid[T->n++] = iid;
        l = next;
    }
    if (!rc && T->n > 1) {                                            /* duplicates: a sorted copy of the names */
        char **sorted = (char **)malloc(sizeof(char *) * (size_t)T->n);
        if (!sorted) rc = HPGV_ERR_NOMEM;
        else {
            memcpy(sorted, T->iid, sizeof(char *) * (size_t)T->n);
            qsort(sorted, (size_t)T->n, sizeof(char *), cmp_iid);
            for (int i = 1; i < T->n && !rc; i++)
                if (!strcmp(sorted[i], sorted[i - 1])) { snprintf(g_err, sizeof g_err, "%s: the id %.200s appears twice", path, sorted[i]); rc = HPGV_ERR_INVALID; }
            free(sorted);
        }
    }
    if (rc) covar_table_free(T);
    return rc;
}

int covar_table_read(const char *path, covar_table_t *T) { return table_read(path, T, "covariate"); }

/* the within file of hpgv_run_assoc_cmh (PLINK's --within): the covariate file's shape and header rule with ONE value column, the
 * cluster's name.  HPGV_ERR_INVALID as above, and for a line with fewer than three tokens (the lines agree in their columns, so a
 * file with none has them all short) and for more than HPGV_CMH_MAX_STRATA distinct names */
int within_table_read(const char *path, covar_table_t *T) {
    int rc = table_read(path, T, "within");
    if (rc) return rc;
    if (T->n > 0 && T->ncols < 1) { snprintf(g_err, sizeof g_err, "%s: a line with fewer than three columns (two ids and a cluster name)", path); rc = HPGV_ERR_INVALID; }
    if (!rc && T->n > 0) {                                            /* the distinct names */
        sample_ids_t *seen = sample_ids_new((size_t)T->n);
        if (!seen) rc = HPGV_ERR_NOMEM;
        int distinct = 0;
        for (int i = 0; !rc && i < T->n; i++)
            if (sample_ids_get(seen, T->c1[i]) < 0) sample_ids_put(seen, T->c1[i], distinct++);
        if (!rc && distinct > HPGV_CMH_MAX_STRATA) { snprintf(g_err, sizeof g_err, "%s: %d clusters, at most %d", path, distinct, (int)HPGV_CMH_MAX_STRATA); rc = HPGV_ERR_INVALID; }
        if (seen) sample_ids_free(seen);
    }
    if (rc) covar_table_free(T);
    return rc;
}

/* stratum[j] for the samples names[0 .. n): the number of the cluster on the line whose second id is names[j] byte for byte, -1
 * without such a line or where take (may be NULL: everyone) has 0 for the sample.  Clusters are numbered by first appearance in
 * the order of names among the samples taken; *n_strata: how many */
int within_table_match(const covar_table_t *T, char *const *names, int n, const uint8_t *take, int32_t *stratum, int *n_strata) {
    sample_ids_t *lines = sample_ids_new((size_t)(T->n > 0 ? T->n : 1)), *clusters = sample_ids_new((size_t)(T->n > 0 ? T->n : 1));
    if (!lines || !clusters) { if (lines) sample_ids_free(lines); if (clusters) sample_ids_free(clusters); return HPGV_ERR_NOMEM; }
    for (int i = 0; i < T->n; i++) sample_ids_put(lines, T->iid[i], i);
    int K = 0;
    for (int j = 0; j < n; j++) {
        stratum[j] = -1;
        if (take && !take[j]) continue;
        const int i = sample_ids_get(lines, names[j]);
        if (i < 0) continue;
        int k = sample_ids_get(clusters, T->c1[i]);
        if (k < 0) { k = K++; sample_ids_put(clusters, T->c1[i], k); }
        stratum[j] = k;
    }
    sample_ids_free(lines); sample_ids_free(clusters);
    *n_strata = K;
    return HPGV_OK;
}

/* how many columns a run uses: n_covar, or every column of the file for 0; -1 (message in g_err) when the file has fewer, or more
 * than HPGV_LOGISTIC_MAX_COVAR are asked for */
int covar_table_columns(const covar_table_t *T, int n_covar) {
    const int use = n_covar > 0 ? n_covar : T->ncols;
    if (n_covar < 0 || use > HPGV_LOGISTIC_MAX_COVAR) { snprintf(g_err, sizeof g_err, "%d covariate columns: at most %d", n_covar > 0 ? n_covar : T->ncols, (int)HPGV_LOGISTIC_MAX_COVAR); return -1; }
    if (use > T->ncols) { snprintf(g_err, sizeof g_err, "%d covariate columns asked for, the file has %d", use, T->ncols); return -1; }
    return use;
}

/* cov[j * stride + k] for the samples names[0 .. n): the first `use` values of the line whose second id is names[j] byte for byte;
 * have[j] = 0 (and zeros in cov) where there is no such line or one of those values is not finite */
int covar_table_match(const covar_table_t *T, char *const *names, int n, int use, double *cov, size_t stride, uint8_t *have) {
    sample_ids_t *ids = sample_ids_new((size_t)(n > 0 ? n : 1));
    if (!ids) return HPGV_ERR_NOMEM;
    for (int j = 0; j < n; j++) { sample_ids_put(ids, names[j], j); have[j] = 0; for (int k = 0; k < use; k++) cov[(size_t)j * stride + (size_t)k] = 0.0; }
    for (int i = 0; i < T->n; i++) {
        const int j = sample_ids_get(ids, T->iid[i]);
        if (j < 0) continue;
        int ok = 1;
        for (int k = 0; k < use; k++) if (!isfinite(T->val[(size_t)i * (size_t)T->ncols + (size_t)k])) ok = 0;
        if (!ok) continue;
        for (int k = 0; k < use; k++) cov[(size_t)j * stride + (size_t)k] = T->val[(size_t)i * (size_t)T->ncols + (size_t)k];
        have[j] = 1;
    }
    sample_ids_free(ids);
    return HPGV_OK;
}

/* the two steps for a caller with its own list of names (the tests): cov has HPGV_LOGISTIC_MAX_COVAR doubles per name */
int hpgv_host_covar_read(const char *covar_path, const char *const *names, int n_names, int n_covar, int *n_covar_out, double *cov, uint8_t *have) {
    if (n_covar_out) *n_covar_out = 0;
    if (!covar_path || n_names < 0 || (n_names > 0 && (!names || !cov || !have))) { snprintf(g_err, sizeof g_err, "bad covariate arguments"); return HPGV_ERR_INVALID; }
    covar_table_t T;
    int rc = covar_table_read(covar_path, &T);
    if (rc) return rc;
    const int use = covar_table_columns(&T, n_covar);
    if (use < 0) rc = HPGV_ERR_INVALID;
    if (!rc) rc = covar_table_match(&T, (char *const *)names, n_names, use, cov, HPGV_LOGISTIC_MAX_COVAR, have);
    if (!rc && n_covar_out) *n_covar_out = use;
    covar_table_free(&T);
    return rc;
}

/* the within file's two steps for a caller with its own list of names (the tests) */
int hpgv_host_within_read(const char *within_path, const char *const *names, int n_names, const uint8_t *take, int32_t *stratum, int *n_strata_out) {
    if (n_strata_out) *n_strata_out = 0;
    if (!within_path || n_names < 0 || !n_strata_out || (n_names > 0 && (!names || !stratum))) { snprintf(g_err, sizeof g_err, "bad within arguments"); return HPGV_ERR_INVALID; }
    covar_table_t T;
    int rc = within_table_read(within_path, &T);
    if (rc) return rc;
    rc = within_table_match(&T, (char *const *)names, n_names, take, stratum, n_strata_out);
    covar_table_free(&T);
    return rc;
}
