/* host_sideout.c -- what a file run keeps beside its result file, and the files written from it at the end: the permutation
 * results (<out>.mperm), the clumping candidates (<out>.clumped), the stats report, the sample pairs of the genome run, the
 * relationship matrix of the GRM run.  Each is
 * a run_*_t of the run with four functions: _new (run_outputs), _add (the writer loop, per written batch), _write and _free (run_finish).
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"

/* the array at *arr (of any element type) grown to cap elements of `size` bytes; 0, and the array as it was, when memory runs out */
static int grown(void *arr, size_t cap, size_t size) {
    void *p;
    memcpy(&p, arr, sizeof p);                           /* (the pointer read and written as bytes: arr is a double **, an int32_t ** ...) */
    if (!(p = realloc(p, cap * size))) return 0;
    memcpy(arr, &p, sizeof p);
    return 1;
}

/* ---- the record heads: "CHR\tPOS\tID" of every kept record, an offset per record into one arena ---------------------- */
int rec_heads_init(rec_heads_t *H, size_t first_cap) {
    memset(H, 0, sizeof *H);
    H->cap = grown(&H->head, first_cap, sizeof *H->head) ? first_cap : 0;
    return !H->cap;
}

int rec_heads_add(rec_heads_t *H, const char *chr, int lc, long pos, const char *id, int li) {
    if (H->n == H->cap) {
        const size_t cap = H->cap ? H->cap * 2 : 1;
        if (!grown(&H->head, cap, sizeof *H->head)) return 1;
        H->cap = cap;
    }
    const size_t need = (size_t)lc + (size_t)li + 32;
    if (H->heads_len + need > H->heads_cap) {
        const size_t cap = (H->heads_cap ? H->heads_cap * 2 : (size_t)1 << 16) + need;
        if (!grown(&H->heads, cap, 1)) return 1;
        H->heads_cap = cap;
    }
    H->head[H->n++] = H->heads_len;                      /* CHR, POS as the result file prints it, ID */
    H->heads_len += (size_t)snprintf(H->heads + H->heads_len, need, "%.*s\t%ld\t%.*s", lc, chr, pos, li, id) + 1;
    return 0;
}

const char *rec_heads_get(const rec_heads_t *H, size_t i) { return H->heads + H->head[i]; }
void rec_heads_free(rec_heads_t *H) { free(H->head); free(H->heads); memset(H, 0, sizeof *H); }

/* CHR, POS and ID of line i of a batch, as rec_heads_add takes them */
typedef struct { const char *chr, *id; int lc, li; long pos; } line_head_t;
static line_head_t line_head(const run_batch_t *b, int i) {
    const uint32_t *fo = b->field_off + 10 * (size_t)i;
    const char *l = b->text + b->line_off[i];
    return (line_head_t){ l + fo[0], l + fo[2], (int)(fo[1] - 1 - fo[0]), (int)(fo[3] - 1 - fo[2]), atol(l + fo[1]) };
}

/* ---- the permutation tools: the records of a written batch kept for <out>.mperm, and that file ---------------------- */
static int run_perm_room(run_perm_t *M) {               /* the parallel arrays as long as the heads' offsets; 0: no memory */
    return grown(&M->t_obs, M->H.cap, sizeof *M->t_obs) & grown(&M->n_ge, M->H.cap, sizeof *M->n_ge);
}

int run_perm_new(run_t *R) {
    run_perm_t *M = R->PM = (run_perm_t *)calloc(1, sizeof *M);
    if (M) M->tmax = (double *)calloc((size_t)R->n_perms, sizeof(double));      /* 0: the identity of the merge */
    return M && M->tmax && !rec_heads_init(&M->H, 4096) && run_perm_room(M) ? HPGV_OK : HPGV_ERR_NOMEM;
}

int run_perm_add(run_t *R, const run_batch_t *b) {
    run_perm_t *M = R->PM;
    const int n = b->n_lines < b->max_lines ? b->n_lines : b->max_lines, m = b->max_lines;
    for (int i = 0; i < n; i++) {
        if (!record_passes(b, i)) continue;
        const line_head_t h = line_head(b, i);
        const size_t k = M->H.n, cap = M->H.cap;
        if (rec_heads_add(&M->H, h.chr, h.lc, h.pos, h.id, h.li) || (M->H.cap != cap && !run_perm_room(M))) return 1;
        M->t_obs[k] = R->tool == RUN_MODEL_PERM ? b->dbl[5 * (size_t)i + HPGV_MODEL_TREND] : R->tool == RUN_LINEAR ? fabs(b->t_obs[i])
                      : run_cmh(R) ? ((const hpgv_cmh_result *)b->dbl)[i].chisq : b->dbl[m + i];
        if (R->tool == RUN_TDT_PERM && M->t_obs[k] < 0) M->t_obs[k] = NAN;      /* chi-square -1: nothing transmitted, no statistic */
        M->n_ge[k] = b->n_ge[i];
    }
    return 0;
}

int run_perm_write(run_t *R, const char *out_path) {
    run_perm_t *M = R->PM;
    const size_t n = M->H.n;
    double *emp = (double *)malloc(sizeof(double) * 2 * (n + 1));
    char *path = (char *)malloc(strlen(out_path) + 8);
    int rc = emp && path ? HPGV_OK : HPGV_ERR_NOMEM;
    if (!rc && (rc = hpgv_perm_pvalues(M->t_obs, (int)n, M->n_ge, M->tmax, R->n_perms, emp, emp + n))) snprintf(g_err, sizeof g_err, "hpgv_perm_pvalues failed (%d)", rc);
    FILE *f = NULL;
    if (!rc) {
        sprintf(path, "%s.mperm", out_path);
        if (!(f = fopen(path, "wb"))) { snprintf(g_err, sizeof g_err, "cannot create %s", path); rc = HPGV_ERR_INVALID; }
    }
    if (!rc) {
        setvbuf(f, NULL, _IOFBF, 1u << 20);
        fputs("#CHR\tPOS\tID\tEMP1\tEMP2\n", f);
        char num[2][320];
        for (size_t i = 0; i < n; i++) {
            hpgv_host_format_f6(emp[i], num[0]); hpgv_host_format_f6(emp[n + i], num[1]);
            if ((R->tool == RUN_LINEAR || run_cmh(R)) && emp[i] != emp[i]) { strcpy(num[0], "nan"); strcpy(num[1], "nan"); }      /* as the run's own columns spell it */
            fprintf(f, "%s\t%s\t%s\n", rec_heads_get(&M->H, i), num[0], num[1]);
        }
        if (fclose(f) != 0) { snprintf(g_err, sizeof g_err, "cannot write %s", path); rc = HPGV_ERR_INVALID; }
        /* the same order as the result file: by chromosome and position (a file in order as written is left alone) */
        else if (hpgv_host_sort_output_file(path)) fprintf(stderr, "WARN: %s could not be sorted by chromosome and position\n", path);
    }
    free(emp); free(path);
    return rc;
}

void run_perm_free(run_t *R) {
    run_perm_t *M = R->PM;
    if (M) { free(M->tmax); free(M->t_obs); free(M->n_ge); rec_heads_free(&M->H); free(M); }
    R->PM = NULL;
}

/* ---- clumping: the candidates of a written batch kept for <out>.clumped, and that file ------------------------------------- */
static int run_clump_room(run_clump_t *M, size_t ns) {   /* the parallel arrays as long as the heads' offsets; 0: no memory */
    return grown(&M->rows, M->H.cap, ns ? ns : 1) & grown(&M->p, M->H.cap, sizeof *M->p)
         & grown(&M->chrom, M->H.cap, sizeof *M->chrom) & grown(&M->pos, M->H.cap, sizeof *M->pos);
}

int run_clump_new(run_t *R) {
    run_clump_t *M = R->CL = (run_clump_t *)calloc(1, sizeof *M);
    return M && !rec_heads_init(&M->H, 1024) && run_clump_room(M, (size_t)R->n_samples) ? HPGV_OK : HPGV_ERR_NOMEM;
}

int run_clump_add(run_t *R, const run_batch_t *b) {
    run_clump_t *M = R->CL;
    const int n = b->n_lines < b->max_lines ? b->n_lines : b->max_lines, m = b->max_lines;
    const size_t ns = (size_t)R->n_samples;
    for (int i = 0; i < n; i++) {
        if (b->sel[i] < 0 || !record_passes(b, i)) continue;       /* (a candidate that only a host-side field filter drops leaves the store here) */
        const line_head_t h = line_head(b, i);
        int ch = -1;                                     /* chromosomes numbered in order of first appearance (a handful of names) */
        for (int k = M->n_chroms - 1; k >= 0 && ch < 0; k--) if ((int)strlen(M->chrom_names[k]) == h.lc && !memcmp(M->chrom_names[k], h.chr, (size_t)h.lc)) ch = k;
        if (ch < 0) {
            if (M->n_chroms == M->chrom_cap) {
                const int cap = M->chrom_cap ? M->chrom_cap * 2 : 32;
                if (!grown(&M->chrom_names, (size_t)cap, sizeof(char *))) return 1;
                M->chrom_cap = cap;
            }
            if (!(M->chrom_names[M->n_chroms] = dupn(h.chr, h.lc))) return 1;
            ch = M->n_chroms++;
        }
        const size_t k = M->H.n, cap = M->H.cap;
        if (rec_heads_add(&M->H, h.chr, h.lc, h.pos, h.id, h.li) || (M->H.cap != cap && !run_clump_room(M, ns))) return 1;
        memcpy(M->rows + k * ns, b->crows + (size_t)b->sel[i] * ns, ns);
        M->p[k] = b->dbl[2 * (size_t)m + (size_t)i];
        M->chrom[k] = ch;
        M->pos[k] = h.pos < 0 ? 0u : h.pos > 0xFFFFFFFFl ? 0xFFFFFFFFu : (uint32_t)h.pos;
    }
    return 0;
}

/* one hpgv_ld_edges over the store (a group: on member 0), hpgv_clump, the file */
int run_clump_write(run_t *R, const char *out_path) {
    run_clump_t *M = R->CL;
    const hpgv_run_clump_options_t *O = R->clump;
    const size_t n = M->H.n;
    int rc = HPGV_OK;
    if (n > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%zu candidates: more than one hpgv_ld_edges call takes", n); return HPGV_ERR_UNSUPPORTED; }
    hpgv_ld_edge *edges = NULL;
    uint64_t n_edges = 0, cap = (uint64_t)n * 4 + 1024;
    hpgv_ctx *ctx = hpgv_group_size(g_ctx) > 1 ? hpgv_group_member(g_ctx, 0) : g_ctx;
    for (int attempt = 0; attempt < 2 && !rc && n > 0; attempt++) {      /* the count exceeds the room: grow and repeat once */
        free(edges);
        if (!(edges = (hpgv_ld_edge *)malloc(sizeof *edges * (size_t)cap))) { rc = HPGV_ERR_NOMEM; break; }
        if ((rc = hpgv_ld_edges(ctx, M->rows, (size_t)R->n_samples, (int)n, O->window, M->chrom, M->pos, O->max_bp, O->min_r2, edges, cap, &n_edges))) {
            snprintf(g_err, sizeof g_err, "hpgv_ld_edges failed (%d): %s", rc, hpgv_last_error(ctx));
            break;
        }
        if (n_edges <= cap) break;
        if (attempt == 1) { snprintf(g_err, sizeof g_err, "hpgv_ld_edges: the number of edges grew between two calls"); rc = HPGV_ERR_INVALID; }
        cap = n_edges;
    }
    int32_t *index_of = (int32_t *)malloc(sizeof(int32_t) * (n + 1)), *order = (int32_t *)malloc(sizeof(int32_t) * (n + 1));
    size_t *first = (size_t *)calloc(n + 2, sizeof(size_t));
    int32_t *member = (int32_t *)malloc(sizeof(int32_t) * (n + 1));
    int n_clumps = 0;
    if (!rc && (!index_of || !order || !first || !member)) rc = HPGV_ERR_NOMEM;
    if (!rc && (rc = hpgv_clump((int)n, M->p, edges, n_edges, O->p1, index_of, order, &n_clumps))) snprintf(g_err, sizeof g_err, "hpgv_clump failed (%d)", rc);
    char *path = (char *)malloc(strlen(out_path) + 12);
    FILE *f = NULL;
    if (!rc && !path) rc = HPGV_ERR_NOMEM;
    if (!rc) {
        sprintf(path, "%s.clumped", out_path);
        if (!(f = fopen(path, "wb"))) { snprintf(g_err, sizeof g_err, "cannot create %s", path); rc = HPGV_ERR_INVALID; }
    }
    if (!rc) {
        /* the claimed members of every index candidate, in file order: counts, offsets, fill */
        for (size_t j = 0; j < n; j++) if (index_of[j] >= 0 && (size_t)index_of[j] != j) first[(size_t)index_of[j] + 1]++;
        for (size_t j = 0; j < n; j++) first[j + 1] += first[j];
        size_t *fill = (size_t *)malloc(sizeof(size_t) * (n + 1));
        if (!fill) rc = HPGV_ERR_NOMEM;
        else {
            memcpy(fill, first, sizeof(size_t) * n);
            for (size_t j = 0; j < n; j++) if (index_of[j] >= 0 && (size_t)index_of[j] != j) member[fill[index_of[j]]++] = (int32_t)j;
            free(fill);
            setvbuf(f, NULL, _IOFBF, 1u << 20);
            fputs("#CHR\tPOS\tID\tP\tTOTAL\tSP2\n", f);
            for (int k = 0; k < n_clumps; k++) {
                const size_t i = (size_t)order[k], total = first[i + 1] - first[i];
                fprintf(f, "%s\t%.6e\t%zu\t", rec_heads_get(&M->H, i), M->p[i], total);
                if (!total) fputs("NONE", f);
                for (size_t q = first[i]; q < first[i + 1]; q++) {
                    const size_t j = (size_t)member[q];
                    fprintf(f, "%s%s:%lu", q > first[i] ? "," : "", M->chrom_names[M->chrom[j]], (unsigned long)atol(strchr(rec_heads_get(&M->H, j), '\t') + 1));
                }
                fputc('\n', f);
            }
        }
        if (fclose(f) != 0 && !rc) { snprintf(g_err, sizeof g_err, "cannot write %s", path); rc = HPGV_ERR_INVALID; }
    }
    /* the candidates whose distance window the candidate window cut short: candidate i + window + 1 is still in reach */
    M->n_clumps = n_clumps; M->n_truncated = 0;
    for (size_t i = 0; !rc && i + (size_t)O->window + 1 < n; i++) {
        const size_t j = i + (size_t)O->window + 1;
        const long long d = (long long)M->pos[j] - (long long)M->pos[i];
        if (M->chrom[j] == M->chrom[i] && (O->max_bp < 0 || (d < 0 ? -d : d) <= O->max_bp)) M->n_truncated++;
    }
    if (!rc && M->n_truncated) fprintf(stderr, "WARN: the window of %d candidates cut the distance window of %ld candidates short\n", O->window, M->n_truncated);
    free(edges); free(index_of); free(order); free(first); free(member); free(path);
    return rc;
}

void run_clump_free(run_t *R) {
    run_clump_t *M = R->CL;
    for (int k = 0; M && k < M->n_chroms; k++) free(M->chrom_names[k]);
    if (M) { free(M->rows); free(M->p); free(M->chrom); free(M->pos); rec_heads_free(&M->H); free(M->chrom_names); free(M); }
    R->CL = NULL;
}

/* ---- sample relatedness: the pair counts of the run on its devices, the expected values' sums, and the file of pairs ---------- */
size_t run_score_bytes(const run_t *R);
static size_t genome_bytes(const run_t *R) {
    if (R->score) return run_score_bytes(R);             /* a score run: its sums and constants, not n x n records */
    const size_t ns = (size_t)R->n_samples, b = ns * ns * sizeof(hpgv_ibs_counts);
    return b ? b : sizeof(hpgv_ibs_counts);
}

int run_genome_new(run_t *R) {
    run_genome_t *G = R->GN = (run_genome_t *)calloc(1, sizeof *G);
    if (!G) return HPGV_ERR_NOMEM;
    const int devs = hpgv_group_size(g_ctx);
    G->n_dev = devs > 1 ? devs : 1;
    G->ctx = (hpgv_ctx **)calloc((size_t)G->n_dev, sizeof *G->ctx);
    G->d_counts = (hpgv_ibs_counts **)calloc((size_t)G->n_dev, sizeof *G->d_counts);
    if (!G->ctx || !G->d_counts) return HPGV_ERR_NOMEM;
    for (int d = 0; d < G->n_dev; d++) {
        G->ctx[d] = devs > 1 ? hpgv_group_member(g_ctx, d) : g_ctx;
        void *p = NULL;
        int rc = hpgv_dev_alloc(G->ctx[d], genome_bytes(R), &p);
        if (rc) { snprintf(g_err, sizeof g_err, "%d samples: no device memory for their %zu bytes of pair counts (%d)", R->n_samples, genome_bytes(R), rc); return rc; }
        G->d_counts[d] = (hpgv_ibs_counts *)p;
        if ((rc = hpgv_memset_dev(G->ctx[d], p, 0, genome_bytes(R), NULL))) return host_fail("hpgv_memset_dev", rc);
    }
    return HPGV_OK;
}

hpgv_ctx *run_genome_device(run_t *R, const run_batch_t *b, hpgv_ibs_counts **d_counts) {
    run_genome_t *G = R->GN;
    int d = 0;
    if (b->dev_text) { for (int k = 0; k < G->n_dev; k++) if (G->ctx[k] == b->dev_ctx) d = k; }      /* (no dev_ctx: the text lies on the first device) */
    else d = (int)(__atomic_fetch_add(&G->next, 1u, __ATOMIC_RELAXED) % (unsigned)G->n_dev);
    *d_counts = G->d_counts[d];
    return G->ctx[d];
}

/* the written records of a batch in file order: a record whose class counts are all zero was a skipped row (chromosome X) and
 * took no part; the terms of the others are added where the row is used */
void run_genome_add(run_t *R, const run_batch_t *b) {
    run_genome_t *G = R->GN;
    const int n = b->n_lines < b->max_lines ? b->n_lines : b->max_lines;
    for (int i = 0; i < n; i++) {
        const int32_t *c = b->ints + 4 * (size_t)i;
        if (!record_passes(b, i) || !(c[0] | c[1] | c[2] | c[3])) continue;
        R->written++;
        double t[5];
        if (!hpgv_ibs_terms(c[0], c[1], c[2], t)) continue;
        G->used++;
        for (int k = 0; k < 5; k++) G->sum[k] += t[k];
    }
}

static int genome_pair_cmp(const void *a, const void *b) {
    const hpgv_ibs_pair *x = (const hpgv_ibs_pair *)a, *y = (const hpgv_ibs_pair *)b;
    return x->i != y->i ? (x->i < y->i ? -1 : 1) : x->j != y->j ? (x->j < y->j ? -1 : 1) : 0;
}

/* the devices' buffers added into the first one's (integers: any order), hpgv_ibs_select_dev there -- once more with room when the
 * list was too short --, the pairs sorted by (i, j), the file */
int run_genome_write(run_t *R, const char *out_path) {
    run_genome_t *G = R->GN;
    const int ns = R->n_samples;
    const size_t bytes = genome_bytes(R);
    int rc = HPGV_OK;
    if (G->n_dev > 1) {
        int32_t *sum = (int32_t *)calloc(bytes / 4, 4), *part = (int32_t *)malloc(bytes);
        if (!sum || !part) rc = HPGV_ERR_NOMEM;
        for (int d = 0; d < G->n_dev && !rc; d++) {
            if ((rc = hpgv_memcpy_d2h(G->ctx[d], part, G->d_counts[d], bytes, NULL))) { host_fail("hpgv_memcpy_d2h", rc); break; }
            for (size_t k = 0; k < bytes / 4; k++) sum[k] += part[k];
        }
        if (!rc && (rc = hpgv_memcpy_h2d(G->ctx[0], G->d_counts[0], sum, bytes, NULL))) host_fail("hpgv_memcpy_h2d", rc);
        free(sum); free(part);
        if (rc) return rc;
    }
    double E[5];
    for (int k = 0; k < 5; k++) E[k] = G->sum[k] / (double)G->used;      /* (no used record: NaN, and no pair qualifies) */
    hpgv_ctx *ctx = G->ctx[0];
    uint64_t cap = (uint64_t)ns * 8 + 16, n = 0;
    hpgv_ibs_pair *pairs = NULL;
    void *d_n = NULL, *d_pairs = NULL;
    if ((rc = hpgv_dev_alloc(ctx, 16, &d_n))) return host_fail("hpgv_dev_alloc", rc);
    for (int attempt = 0; attempt < 2 && !rc; attempt++) {      /* the count exceeds the room: grow and repeat once */
        if ((rc = hpgv_dev_alloc(ctx, (size_t)cap * sizeof(hpgv_ibs_pair), &d_pairs))) { host_fail("hpgv_dev_alloc", rc); break; }
        if ((rc = hpgv_ibs_select_dev(ctx, G->d_counts[0], ns, E, R->min_pi_hat, (hpgv_ibs_pair *)d_pairs, cap, (uint64_t *)d_n, NULL)) ||
            (rc = hpgv_memcpy_d2h(ctx, &n, d_n, sizeof n, NULL))) {
            snprintf(g_err, sizeof g_err, "hpgv_ibs_select_dev failed (%d): %s", rc, hpgv_last_error(ctx));
        } else if (n <= cap) {
            if (!(pairs = (hpgv_ibs_pair *)malloc(sizeof *pairs * (size_t)(n + 1)))) rc = HPGV_ERR_NOMEM;
            else if (n && (rc = hpgv_memcpy_d2h(ctx, pairs, d_pairs, (size_t)n * sizeof *pairs, NULL))) host_fail("hpgv_memcpy_d2h", rc);
        } else if (attempt == 1) { snprintf(g_err, sizeof g_err, "hpgv_ibs_select_dev: the number of pairs grew between two calls"); rc = HPGV_ERR_INVALID; }
        (void)hpgv_dev_free(ctx, d_pairs);
        if (pairs || rc) break;
        cap = n;
    }
    (void)hpgv_dev_free(ctx, d_n);
    FILE *f = NULL;
    if (!rc && !(f = fopen(out_path, "wb"))) { snprintf(g_err, sizeof g_err, "cannot create %s", out_path); rc = HPGV_ERR_INVALID; }
    if (!rc) {
        qsort(pairs, (size_t)n, sizeof *pairs, genome_pair_cmp);
        setvbuf(f, NULL, _IOFBF, 1u << 20);
        fputs("#IID1\tIID2\tNM\tIBS0\tIBS1\tIBS2\tZ0\tZ1\tZ2\tPI_HAT\tDST\n", f);
        char num[5][320];
        for (uint64_t q = 0; q < n; q++) {
            const hpgv_ibs_pair *p = pairs + q;
            double g[5];
            hpgv_ibs_genome(&p->c, E, g);
            for (int k = 0; k < 5; k++) hpgv_host_format_f6(g[k], num[k]);
            fprintf(f, "%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%s\t%s\n", R->names[p->i], R->names[p->j], p->c.n, p->c.ibs0, p->c.ibs1, p->c.ibs2,
                    num[0], num[1], num[2], num[3], num[4]);
        }
        if (fclose(f) != 0) { snprintf(g_err, sizeof g_err, "cannot write %s", out_path); rc = HPGV_ERR_INVALID; }
        else G->n_pairs = (long)n;
    }
    free(pairs);
    return rc;
}

void run_genome_free(run_t *R) {
    run_genome_t *G = R->GN;
    for (int d = 0; G && G->d_counts && G->ctx && d < G->n_dev; d++) if (G->d_counts[d]) (void)hpgv_dev_free(G->ctx[d], G->d_counts[d]);
    if (G) { free(G->ctx); free(G->d_counts); free(G); }
    R->GN = NULL;
}

/* ---- genetic relationship matrix: the pair sums of the run lie in the genome run's device buffers (run_genome_new / _device /
 *      _free: one n_samples x n_samples buffer of 16-byte records per device, whichever record) ---------------------------------- */
_Static_assert(sizeof(hpgv_grm_acc) == sizeof(hpgv_ibs_counts), "the GRM run keeps its sums in run_genome_t's buffers");

/* the written records of a batch: a record whose class counts are all zero was a skipped row; the run counts the USED ones, by the
 * function the device's table kernel is */
void run_grm_add(run_t *R, const run_batch_t *b) {
    const int n = b->n_lines < b->max_lines ? b->n_lines : b->max_lines;
    for (int i = 0; i < n; i++) {
        const int32_t *c = b->ints + 4 * (size_t)i;
        int8_t hi[4], lo[4];
        if (!record_passes(b, i) || !(c[0] | c[1] | c[2] | c[3])) continue;
        if (hpgv_grm_table(c[0], c[1], c[2], R->frac_bits, R->min_maf, hi, lo)) R->written++;
    }
}

int grm_put(const char *prefix, const char *suffix, const void *data, size_t bytes) {
    char *path = (char *)malloc(strlen(prefix) + strlen(suffix) + 1);
    if (!path) return HPGV_ERR_NOMEM;
    strcpy(path, prefix); strcat(path, suffix);
    FILE *f = fopen(path, "wb");
    int rc = HPGV_OK;
    if (!f) { snprintf(g_err, sizeof g_err, "cannot create %s", path); rc = HPGV_ERR_INVALID; }
    else if ((fwrite(data, 1, bytes, f) != bytes) | (fclose(f) != 0)) { snprintf(g_err, sizeof g_err, "cannot write %s", path); rc = HPGV_ERR_INVALID; }
    free(path);
    return rc;
}

/* the devices' sums added as integers (any order): *sum_out, n_samples x n_samples records, the caller's to free */
int run_grm_sum(run_t *R, hpgv_grm_acc **sum_out) {
    run_genome_t *G = R->GN;
    const size_t ns = (size_t)R->n_samples, recs = ns * ns;
    int rc = HPGV_OK;
    hpgv_grm_acc *sum = (hpgv_grm_acc *)calloc(recs ? recs : 1, sizeof *sum), *part = G->n_dev > 1 ? (hpgv_grm_acc *)malloc((recs ? recs : 1) * sizeof *part) : NULL;
    if (!sum || (G->n_dev > 1 && !part)) rc = HPGV_ERR_NOMEM;
    for (int d = 0; d < G->n_dev && !rc && recs; d++) {
        hpgv_grm_acc *to = d == 0 ? sum : part;
        if ((rc = hpgv_memcpy_d2h(G->ctx[d], to, G->d_counts[d], recs * sizeof *to, NULL))) { host_fail("hpgv_memcpy_d2h", rc); break; }
        for (size_t k = 0; d > 0 && k < recs; k++) { sum[k].sq += part[k].sq; sum[k].n += part[k].n; }
    }
    free(part);
    if (rc) { free(sum); sum = NULL; }
    *sum_out = sum;
    return rc;
}

/* GCTA's binary triplet of the summed records: <prefix>.grm.bin, float32 of hpgv_grm_value for rows i = 0 .. n - 1 and columns
 * j = 0 .. i (the record lies at [min][max]); <prefix>.grm.N.bin, float32 of n in the same order; <prefix>.grm.id,
 * "name<TAB>name" per sample */
int run_grm_files(run_t *R, const char *out_prefix, const hpgv_grm_acc *sum) {
    const size_t ns = (size_t)R->n_samples, tri = ns * (ns + 1) / 2;
    int rc = HPGV_OK;
    float *val = (float *)malloc((tri ? tri : 1) * sizeof *val), *cnt = (float *)malloc((tri ? tri : 1) * sizeof *cnt);
    if (!val || !cnt) rc = HPGV_ERR_NOMEM;
    if (!rc) {
        size_t at = 0;
        for (size_t i = 0; i < ns; i++)
            for (size_t j = 0; j <= i; j++, at++) {
                const hpgv_grm_acc *a = sum + j * ns + i;
                val[at] = (float)hpgv_grm_value(a, R->frac_bits);
                cnt[at] = (float)a->n;
            }
        rc = grm_put(out_prefix, ".grm.bin", val, tri * sizeof *val);
        if (!rc) rc = grm_put(out_prefix, ".grm.N.bin", cnt, tri * sizeof *cnt);
    }
    if (!rc) {
        size_t len = 0;
        for (size_t j = 0; j < ns; j++) len += 2 * strlen(R->names[j]) + 2;
        char *ids = (char *)malloc(len + 1), *w = ids;
        if (!ids) rc = HPGV_ERR_NOMEM;
        for (size_t j = 0; j < ns && !rc; j++) w += sprintf(w, "%s\t%s\n", R->names[j], R->names[j]);
        if (!rc) rc = grm_put(out_prefix, ".grm.id", ids, (size_t)(w - ids));
        free(ids);
    }
    free(val); free(cnt);
    return rc;
}

int run_grm_write(run_t *R, const char *out_prefix) {
    hpgv_grm_acc *sum = NULL;
    int rc = run_grm_sum(R, &sum);
    if (!rc) rc = run_grm_files(R, out_prefix, sum);
    free(sum);
    return rc;
}

/* ---- allele scoring (include/hpgv.h "Score"): a GRM-shaped run with a score plan (run_t::score) -- the score file's ids in a hash,
 *      the callback that weighs a batch's lines by them, the devices' sums added on the host, and the .profile.  The sums of a
 *      device lie in the genome run's buffer of that device: (n_scores + 2) x acc_pitch int64, then the n_scores + 1 constants -- */
size_t run_score_acc_pitch(const run_t *R) { return ((size_t)(R->n_samples > 0 ? R->n_samples : 1) + 1) / 2 * 2; }
static size_t score_words(const run_t *R) { return ((size_t)R->score->n_scores + 2) * run_score_acc_pitch(R) + (size_t)R->score->n_scores + 1; }

static uint64_t score_hash(const char *s, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;                  /* FNV-1a */
    for (size_t i = 0; i < n; i++) h = (h ^ (unsigned char)s[i]) * 0x100000001B3ull;
    return h;
}

/* the line of the id s[0 .. n), or -1; add >= 0: the id goes in as line `add` when it is new (-2: it was there) */
static long score_find(run_score_t *S, const char *s, size_t n, long add) {
    for (size_t at = (size_t)score_hash(s, n) & S->mask; ; at = (at + 1) & S->mask) {
        const long k = S->slot[at];
        if (k < 0) { if (add >= 0) S->slot[at] = add; return -1; }
        if (strlen(S->id[k]) == n && !memcmp(S->id[k], s, n)) return add >= 0 ? -2 : k;
    }
}

void run_score_free(run_score_t *S) {
    if (!S) return;
    free(S->blob); free(S->id); free(S->allele); free(S->w); free(S->slot); free(S->name);
    memset(S, 0, sizeof *S);
}

static int score_is_space(char c) { return c == ' ' || c == '\t' || c == '\r'; }

/* the score file: whitespace-separated id, allele and 1 .. HPGV_SCORE_MAX weights per line, the same number on every line; a first
 * line whose first token is ID, #ID or SNP names the columns.  frac_bits[k] = hpgv_score_frac_bits of column k's largest |w| */
int run_score_read(const char *path, int impute, run_score_t *S) {
    memset(S, 0, sizeof *S);
    S->impute = impute != 0;
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(g_err, sizeof g_err, "cannot open score file %s", path); return HPGV_ERR_INVALID; }
    size_t len = 0, cap = 1u << 16;
    char *blob = (char *)malloc(cap + 1);
    for (size_t got; blob && (got = fread(blob + len, 1, cap - len, f)) > 0; ) {
        len += got;
        if (len == cap) { char *nb = (char *)realloc(blob, (cap *= 2) + 1); if (!nb) { free(blob); } blob = nb; }
    }
    const int io_bad = ferror(f);
    fclose(f);
    if (!blob) return HPGV_ERR_NOMEM;
    if (io_bad) { free(blob); snprintf(g_err, sizeof g_err, "cannot read score file %s", path); return HPGV_ERR_INVALID; }
    blob[len] = 0;
    S->blob = blob;
    size_t n_lines = 1;
    for (size_t i = 0; i < len; i++) n_lines += blob[i] == '\n';
    S->id = (char **)calloc(n_lines, sizeof *S->id); S->allele = (char **)calloc(n_lines, sizeof *S->allele);
    size_t slots = 16;
    while (slots < 2 * n_lines) slots *= 2;
    S->slot = (long *)malloc(slots * sizeof *S->slot); S->mask = slots - 1;
    S->name = (char (*)[64])calloc(HPGV_SCORE_MAX, sizeof S->name[0]);
    if (!S->id || !S->allele || !S->slot || !S->name) { run_score_free(S); return HPGV_ERR_NOMEM; }
    for (size_t i = 0; i < slots; i++) S->slot[i] = -1;
    int rc = HPGV_OK, first = 1;
    double big[HPGV_SCORE_MAX] = { 0 };
    char *tok[HPGV_SCORE_MAX + 3];
    for (char *line = blob, *end = blob + len, *next; line < end && !rc; line = next) {
        char *nl = (char *)memchr(line, '\n', (size_t)(end - line));
        next = nl ? nl + 1 : end;
        if (nl) *nl = 0;
        int nt = 0;
        for (char *c = line; *c; ) {
            while (score_is_space(*c)) *c++ = 0;
            if (!*c) break;
            if (nt < HPGV_SCORE_MAX + 3) tok[nt] = c;
            nt++;
            while (*c && !score_is_space(*c)) c++;
        }
        if (nt == 0) continue;                           /* an empty line */
        const long line_no = S->n + (S->have_header ? 2 : 1);
        if (nt > HPGV_SCORE_MAX + 2) { snprintf(g_err, sizeof g_err, "%s: line %ld has %d weight columns, at most %d", path, line_no, nt - 2, HPGV_SCORE_MAX); rc = HPGV_ERR_INVALID; break; }
        if (nt < 3) { snprintf(g_err, sizeof g_err, "%s: line %ld has %d columns: id, allele and at least one weight", path, line_no, nt); rc = HPGV_ERR_INVALID; break; }
        if (first) {
            first = 0;
            S->n_scores = nt - 2;
            S->w = (double *)malloc(n_lines * (size_t)S->n_scores * sizeof *S->w);
            if (!S->w) { rc = HPGV_ERR_NOMEM; break; }
            S->have_header = !strcmp(tok[0], "ID") || !strcmp(tok[0], "#ID") || !strcmp(tok[0], "SNP");
            for (int k = 0; k < S->n_scores; k++) {
                if (S->have_header) snprintf(S->name[k], sizeof S->name[k], "%.*s", (int)sizeof S->name[k] - 1, tok[2 + k]);
                else snprintf(S->name[k], sizeof S->name[k], "SCORE%d", k + 1);
            }
            if (S->have_header) continue;
        }
        if (nt - 2 != S->n_scores) { snprintf(g_err, sizeof g_err, "%s: line %ld has %d weight columns, the first line %d", path, line_no, nt - 2, S->n_scores); rc = HPGV_ERR_INVALID; break; }
        if (score_find(S, tok[0], strlen(tok[0]), S->n) == -2) { snprintf(g_err, sizeof g_err, "%s: line %ld: the id %.100s appears twice", path, line_no, tok[0]); rc = HPGV_ERR_INVALID; break; }
        S->id[S->n] = tok[0]; S->allele[S->n] = tok[1];
        for (int k = 0; k < S->n_scores; k++) {
            char *e = NULL;
            const double v = strtod(tok[2 + k], &e);
            if (e == tok[2 + k] || *e || !isfinite(v)) { snprintf(g_err, sizeof g_err, "%s: line %ld: the weight %.100s is not a finite number", path, line_no, tok[2 + k]); rc = HPGV_ERR_INVALID; break; }
            S->w[(size_t)S->n * (size_t)S->n_scores + (size_t)k] = v;
            if (fabs(v) > big[k]) big[k] = fabs(v);
        }
        S->n++;
    }
    if (!rc && S->n == 0) { snprintf(g_err, sizeof g_err, "%s holds no line of weights", path); rc = HPGV_ERR_INVALID; }
    for (int k = 0; k < S->n_scores && !rc; k++) S->frac_bits[k] = hpgv_score_frac_bits(big[k]);
    if (rc) run_score_free(S);
    return rc;
}

/* hpgv_score_text's callback (on the engine thread that made the call): a record takes part when its id is in the file and the
 * file's allele is its ALT (byte for byte) or its REF (the row is flipped); a record with a ',' in ALT, with the id "." or an id
 * that is not in the file is skipped; one whose allele is neither REF nor ALT is skipped and counted */
int run_score_weigh(void *user, const char *text, int n_lines, const uint64_t *line_off, const uint32_t *field_off, const int32_t *status,
                    double *w, uint8_t *flags) {
    run_score_t *S = (run_score_t *)user;
    long unmatched = 0;
    for (int i = 0; i < n_lines; i++) {
        const uint32_t *fo = field_off + 10 * (size_t)i;
        flags[i] = HPGV_SCORE_SKIP;
        if ((status[i] & 0xFF) == 1 || fo[5] == 0xFFFFFFFFu) continue;
        const char *l = text + line_off[i];
        const char *id = l + fo[2], *ref = l + fo[3], *alt = l + fo[4];
        const size_t n_id = fo[3] - 1 - fo[2], n_ref = fo[4] - 1 - fo[3], n_alt = fo[5] - 1 - fo[4];
        if (memchr(alt, ',', n_alt) || (n_id == 1 && id[0] == '.')) continue;
        const long k = score_find(S, id, n_id, -1);
        if (k < 0) continue;
        const size_t n_a = strlen(S->allele[k]);
        if (n_a == n_alt && !memcmp(S->allele[k], alt, n_alt)) flags[i] = 0;
        else if (n_a == n_ref && !memcmp(S->allele[k], ref, n_ref)) flags[i] = HPGV_SCORE_FLIP;
        else { unmatched++; continue; }
        memcpy(w + (size_t)i * (size_t)S->n_scores, S->w + (size_t)k * (size_t)S->n_scores, (size_t)S->n_scores * sizeof *w);
    }
    if (unmatched) __atomic_fetch_add(&S->n_unmatched, unmatched, __ATOMIC_RELAXED);
    return 0;
}

size_t run_score_bytes(const run_t *R) { return score_words(R) * sizeof(int64_t); }

/* the devices' sums and constants added as integers (any order): *sum_out, score_words of them, the caller's to free */
int run_score_sum(run_t *R, int64_t **sum_out) {
    run_genome_t *G = R->GN;
    const size_t words = score_words(R);
    int rc = HPGV_OK;
    int64_t *sum = (int64_t *)calloc(words, sizeof *sum), *part = G->n_dev > 1 ? (int64_t *)malloc(words * sizeof *part) : NULL;
    if (!sum || (G->n_dev > 1 && !part)) rc = HPGV_ERR_NOMEM;
    for (int d = 0; d < G->n_dev && !rc; d++) {
        int64_t *to = d == 0 ? sum : part;
        if ((rc = hpgv_memcpy_d2h(G->ctx[d], to, G->d_counts[d], words * sizeof *to, NULL))) { host_fail("hpgv_memcpy_d2h", rc); break; }
        for (size_t k = 0; d > 0 && k < words; k++) sum[k] += part[k];
    }
    free(part);
    if (rc) { free(sum); sum = NULL; }
    *sum_out = sum;
    return rc;
}

static void score_put_g8(FILE *f, double v) {
    if (v != v) fputs("\tnan", f);                       /* (whichever NaN) */
    else fprintf(f, "\t%.8g", v);
}

/* the .profile: "#FID IID CNT CNT2" and <name>_SUM, <name>_AVG per score, one line per sample in VCF order */
int run_score_write(run_t *R, const char *out_path) {
    const run_score_t *S = R->score;
    const size_t ns = (size_t)R->n_samples, pitch = run_score_acc_pitch(R);
    const int K = S->n_scores;
    int64_t *sum = NULL;
    int rc = run_score_sum(R, &sum);
    if (rc) return rc;
    const int64_t *cnst = sum + ((size_t)K + 2) * pitch, n_used = cnst[K];
    R->written = (long)n_used;
    FILE *f = fopen(out_path, "wb");
    if (!f) { snprintf(g_err, sizeof g_err, "cannot create %s", out_path); free(sum); return HPGV_ERR_INVALID; }
    setvbuf(f, NULL, _IOFBF, 1u << 20);
    fputs("#FID\tIID\tCNT\tCNT2", f);
    for (int k = 0; k < K; k++) fprintf(f, "\t%s_SUM\t%s_AVG", S->name[k], S->name[k]);
    fputc('\n', f);
    for (size_t j = 0; j < ns; j++) {
        const int64_t n = S->impute ? n_used : sum[(size_t)K * pitch + j];
        fprintf(f, "%s\t%s\t%lld\t%lld", R->names[j], R->names[j], (long long)(2 * n), (long long)sum[((size_t)K + 1) * pitch + j]);
        for (int k = 0; k < K; k++) {
            const double v = hpgv_score_value(sum[(size_t)k * pitch + j], cnst[k], S->frac_bits[k]);
            score_put_g8(f, v);
            score_put_g8(f, v / (2.0 * (double)n));
        }
        fputc('\n', f);
    }
    if ((ferror(f) != 0) | (fclose(f) != 0)) { snprintf(g_err, sizeof g_err, "cannot write %s", out_path); rc = HPGV_ERR_INVALID; }
    free(sum);
    return rc;
}

/* ---- hpg-var-vcf stats: what the run accumulates besides the per-variant lines (run_stats_t; the report writers live in
 *      hpg-libs, so the two files below are this project's rendering) ---- */
int run_stats_new(run_t *R) {
    run_stats_t *RS = R->RS = (run_stats_t *)calloc(1, sizeof *RS);
    if (RS) { RS->smiss = (long *)calloc((size_t)R->n_samples + 1, sizeof(long)); RS->serr = (long *)calloc((size_t)R->n_samples + 1, sizeof(long)); }
    return RS && RS->smiss && RS->serr ? HPGV_OK : HPGV_ERR_NOMEM;
}

/* the per-phenotype lines of a batch: the counters of the first two alleles within the group (variant_stats_t per
 * phenotype, stats_runner.c:319-323) */
static void write_group_lines(FILE **gfd, const run_batch_t *b) {
    const int n = b->n_lines < b->max_lines ? b->n_lines : b->max_lines, m = b->max_lines;
    for (int g = 0; g < b->n_groups; g++)
        for (int i = 0; i < n; i++) {
            if (!record_passes(b, i)) continue;
            const uint32_t *fo = b->field_off + 10 * (size_t)i;
            const char *l = b->text + b->line_off[i];
            const int32_t *c = b->gc8 + ((size_t)g * m + (size_t)i) * 8;
            const int ta = c[6] + c[7];
            const float f0 = ta ? (float)c[6] / ta : 0.0f, f1 = ta ? (float)c[7] / ta : 0.0f;
            fprintf(gfd[g], "%.*s\t%ld\t%.*s\t%.*s\t%d,%d\t%.4f,%.4f\t0/0:%d,0/1:%d,1/1:%d,./.:%d\t%d\t%d\t%.4f\t%.6g\t%.6g\n",
                    (int)(fo[1] - 1 - fo[0]), l + fo[0], atol(l + fo[1]), (int)(fo[4] - 1 - fo[3]), l + fo[3], (int)(fo[5] - 1 - fo[4]), l + fo[4],
                    c[6], c[7], f0, f1, c[0], c[1] + c[2], c[3], c[4], c[5], c[4], f0 < f1 ? f0 : f1,
                    b->ghw[(size_t)g * m + (size_t)i], b->ghw[((size_t)b->n_groups + (size_t)g) * m + (size_t)i]);
        }
}

void run_stats_add(run_t *run, const run_batch_t *b) {
    run_stats_t *R = run->RS;
    for (int j = 0; j < run->n_samples; j++) R->smiss[j] += b->smiss[j];      /* counted over every line of the batch, as get_sample_stats does */
    for (int t = 0; t < b->n_cerr; t++) R->serr[run->trio_child[t]] += b->cerr[t];
    const int n = b->n_lines < b->max_lines ? b->n_lines : b->max_lines;
    for (int i = 0; i < n; i++) {
        if (!record_passes(b, i)) continue;
        const uint32_t *fo = b->field_off + 10 * (size_t)i;
        const char *l = b->text + b->line_off[i];
        const char *ref = l + fo[3], *alt = l + fo[4];
        const int lr = (int)(fo[4] - 1 - fo[3]), la = (int)(fo[5] - 1 - fo[4]);
        vcounts_t v;
        record_counts(b, i, alt, la, &v);
        R->variants++;
        if (v.na > 2) R->multiallelic++; else R->biallelic++;
        int snp = lr == 1, n_alt = 0;                      /* a SNP: REF and every ALT allele one base long */
        for (int k = 0, start = 0; k <= la; k++)
            if (k == la || alt[k] == ',') { n_alt++; if (k - start != 1 || alt[start] == '.') snp = 0; start = k + 1; }
        if (snp) {
            R->snps++;
            if (n_alt == 1) {
                const char a = (char)(ref[0] & ~0x20), c = (char)(alt[0] & ~0x20);
                const int purine_a = a == 'A' || a == 'G', purine_c = c == 'A' || c == 'G';
                if (purine_a == purine_c) R->transitions++; else R->transversions++;
            }
        } else if (!(la == 1 && alt[0] == '.')) R->indels++;
        if (fo[6] != 0xFFFFFFFFu) {
            const char *q = l + fo[5];
            if (*q != '.' && *q != '\t') { R->quality_sum += strtod(q, NULL); R->with_quality++; }
            const char *f = l + fo[6];
            const int lf = fo[7] != 0xFFFFFFFFu ? (int)(fo[7] - 1 - fo[6]) : 0;
            if (lf == 4 && !strncmp(f, "PASS", 4)) R->pass++;
        }
    }
    if (run->gfd) write_group_lines(run->gfd, b);         /* (the group files: by the writer loop's thread) */
}

int run_stats_write(const run_t *run, const char *prefix) {
    const run_stats_t *R = run->RS;
    const int n_samples = run->n_samples;
    char *path = (char *)malloc(strlen(prefix) + 32);
    if (!path) return HPGV_ERR_NOMEM;
    sprintf(path, "%s.stats-samples", prefix);
    FILE *f = fopen(path, "w");
    if (!f) goto fail;
    fprintf(f, "#SAMPLE\tMISS_GT\tMEND_ER\n");
    for (int j = 0; j < n_samples; j++) fprintf(f, "%s\t%ld\t%ld\n", run->names[j], R->smiss[j], R->serr[j]);
    fclose(f);
    sprintf(path, "%s.stats-summary", prefix);
    if (!(f = fopen(path, "w"))) goto fail;
    fprintf(f, "Number of variants = %ld\nNumber of samples = %d\nNumber of biallelic variants = %ld\nNumber of multiallelic variants = %ld\n\n",
            run->written, n_samples, R->biallelic, R->multiallelic);
    fprintf(f, "Number of SNP = %ld\nNumber of indels = %ld\n\n", R->snps, R->indels);
    fprintf(f, "Number of transitions = %ld\nNumber of transversions = %ld\nTi/TV ratio = %.4f\n\n", R->transitions, R->transversions,
            R->transversions ? (double)R->transitions / (double)R->transversions : 0.0);
    fprintf(f, "Percentage of PASS = %.2f%%\nAverage quality = %.2f\n", R->variants ? 100.0 * (double)R->pass / (double)R->variants : 0.0,
            R->with_quality ? R->quality_sum / (double)R->with_quality : 0.0);
    fclose(f);
    free(path);
    return HPGV_OK;
fail:
    snprintf(g_err, sizeof g_err, "cannot create %s", path); free(path); return HPGV_ERR_INVALID;
}

void run_stats_free(run_t *R) {
    if (R->RS) { free(R->RS->smiss); free(R->RS->serr); free(R->RS); }
    R->RS = NULL;
}
