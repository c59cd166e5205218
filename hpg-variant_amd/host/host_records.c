/* host_records.c -- the record filters of hpgv_run_set_record_filters (shared_options.c:42-56,86-173): --region,
 * --region-file / --region-type, --coverage, --snp, --var-type, --indel from the line heads, and the thresholds of the
 * device-side --inh-dom / --inh-rec.  A setting is parsed once, when it is set, into an immutable object that every run
 * started afterwards holds a reference to.
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"
#include <errno.h>
#include <limits.h>

/* INFO's DP as atoi reads it: the first ';'-separated entry whose key is exactly DP; optional sign, then digits up to the
 * first non-digit, none giving 0, saturated at the int64 range.  0 when there is no such entry or it is a bare flag. */
int info_dp(const char *info, size_t n, long long *v) {
    size_t k = 0;
    while (k <= n) {
        size_t e = k;
        while (e < n && info[e] != ';') e++;
        if (e - k >= 2 && info[k] == 'D' && info[k + 1] == 'P' && (e - k == 2 || info[k + 2] == '=')) {
            if (e - k == 2) return 0;                         /* a bare flag */
            size_t q = k + 3;
            int neg = 0;
            if (q < e && (info[q] == '-' || info[q] == '+')) neg = info[q++] == '-';
            unsigned long long m = 0, lim = neg ? (unsigned long long)LLONG_MAX + 1ull : (unsigned long long)LLONG_MAX;
            for (; q < e && info[q] >= '0' && info[q] <= '9'; q++) {
                const unsigned d = (unsigned)(info[q] - '0');
                m = m > (lim - d) / 10 ? lim : m * 10 + d;
            }
            *v = neg ? (m == (unsigned long long)LLONG_MAX + 1ull ? LLONG_MIN : -(long long)m) : (long long)m;
            return 1;
        }
        k = e + 1;
    }
    return 0;
}

/* INFO of line i of a batch (the heads hold it whatever the text's residence): 0 when the line has no INFO field */
int record_info(const run_batch_t *b, int i, const char **info, size_t *n) {
    const uint32_t *fo = b->field_off + 10 * (size_t)i;
    if (fo[7] == 0xFFFFFFFFu) return 0;
    const char *l = b->text + b->line_off[i];
    size_t ie = fo[8] != 0xFFFFFFFFu ? (size_t)fo[8] - 1 : (size_t)(b->line_off[i + 1] - b->line_off[i]);
    if (fo[8] == 0xFFFFFFFFu && ie > fo[7] && l[ie - 1] == '\n') ie--;
    *info = l + fo[7]; *n = ie > fo[7] ? ie - fo[7] : 0;
    return 1;
}

/* ---- regions: per sequence, sorted and merged 1-based inclusive intervals ---- */
typedef struct { char *name; size_t len; long *iv; int n, cap; } reg_seq_t;
typedef struct { reg_seq_t *s; int n, cap; } reg_set_t;

static void reg_free(reg_set_t *R) {
    for (int k = 0; k < R->n; k++) { free(R->s[k].name); free(R->s[k].iv); }
    free(R->s);
    memset(R, 0, sizeof *R);
}

static int reg_add(reg_set_t *R, const char *name, size_t len, long lo, long hi) {
    reg_seq_t *q = NULL;
    for (int k = R->n - 1; k >= 0 && !q; k--) if (R->s[k].len == len && !memcmp(R->s[k].name, name, len)) q = &R->s[k];
    if (!q) {
        if (R->n == R->cap) {
            const int c = R->cap ? 2 * R->cap : 16;
            reg_seq_t *s = (reg_seq_t *)realloc(R->s, sizeof *s * (size_t)c);
            if (!s) return HPGV_ERR_NOMEM;
            R->s = s; R->cap = c;
        }
        q = &R->s[R->n];
        memset(q, 0, sizeof *q);
        if (!(q->name = (char *)malloc(len + 1))) return HPGV_ERR_NOMEM;
        memcpy(q->name, name, len); q->name[len] = 0; q->len = len;
        R->n++;
    }
    if (q->n == q->cap) {
        const int c = q->cap ? 2 * q->cap : 8;
        long *iv = (long *)realloc(q->iv, sizeof(long) * 2 * (size_t)c);
        if (!iv) return HPGV_ERR_NOMEM;
        q->iv = iv; q->cap = c;
    }
    q->iv[2 * q->n] = lo; q->iv[2 * q->n + 1] = hi; q->n++;
    return HPGV_OK;
}

static int cmp_iv(const void *a, const void *b) {
    const long x = *(const long *)a, y = *(const long *)b;
    return x < y ? -1 : x > y;
}
static int cmp_seq(const void *a, const void *b) {
    const reg_seq_t *x = (const reg_seq_t *)a, *y = (const reg_seq_t *)b;
    const int c = memcmp(x->name, y->name, x->len < y->len ? x->len : y->len);
    return c ? c : (x->len < y->len ? -1 : x->len > y->len);
}
/* sequences by name, each one's intervals by start and merged where they overlap or touch */
static void reg_finish(reg_set_t *R) {
    qsort(R->s, (size_t)R->n, sizeof *R->s, cmp_seq);
    for (int k = 0; k < R->n; k++) {
        reg_seq_t *q = &R->s[k];
        qsort(q->iv, (size_t)q->n, 2 * sizeof(long), cmp_iv);
        int m = 0;
        for (int j = 0; j < q->n; j++) {
            const long lo = q->iv[2 * j], hi = q->iv[2 * j + 1];
            if (m > 0 && (q->iv[2 * m - 1] == LONG_MAX || lo <= q->iv[2 * m - 1] + 1)) { if (hi > q->iv[2 * m - 1]) q->iv[2 * m - 1] = hi; }
            else { q->iv[2 * m] = lo; q->iv[2 * m + 1] = hi; m++; }
        }
        q->n = m;
    }
}

static int reg_has(const reg_set_t *R, const char *name, size_t len, long pos) {
    int lo = 0, hi = R->n;
    const reg_seq_t key = { (char *)name, len, NULL, 0, 0 };
    while (lo < hi) {                                     /* the sequence */
        const int mid = (lo + hi) >> 1, c = cmp_seq(&R->s[mid], &key);
        if (c == 0) { lo = mid; hi = -1; break; }
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    if (hi != -1) return 0;
    const reg_seq_t *q = &R->s[lo];
    int a = 0, b = q->n;                                  /* the last interval starting at or before pos */
    while (a < b) { const int mid = (a + b) >> 1; if (q->iv[2 * mid] <= pos) a = mid + 1; else b = mid; }
    return a > 0 && pos <= q->iv[2 * (a - 1) + 1];
}

/* a position: one or more decimal digits, at least `min`, within the long range */
static int parse_pos(const char *p, size_t n, long min, long *v) {
    if (n == 0 || n > 19) return 0;
    long x = 0;
    for (size_t k = 0; k < n; k++) {
        if (p[k] < '0' || p[k] > '9') return 0;
        if (x > (LONG_MAX - (p[k] - '0')) / 10) return 0;
        x = x * 10 + (p[k] - '0');
    }
    if (x < min) return 0;
    *v = x;
    return 1;
}

/* --region: CHROM | CHROM:POS | CHROM:START-END, comma-separated; the last ':' of an item separates CHROM */
static int parse_regions(const char *text, reg_set_t *R) {
    const char *p = text;
    for (;;) {
        const char *e = strchr(p, ',');
        const size_t n = e ? (size_t)(e - p) : strlen(p);
        const char *colon = NULL;
        for (size_t k = 0; k < n; k++) if (p[k] == ':') colon = p + k;
        long lo = LONG_MIN, hi = LONG_MAX;
        const size_t cl = colon ? (size_t)(colon - p) : n;
        int ok = cl > 0;
        if (ok && colon) {
            const char *r = colon + 1, *end = p + n, *dash = (const char *)memchr(r, '-', (size_t)(end - r));
            if (!dash) { ok = parse_pos(r, (size_t)(end - r), 1, &lo); hi = lo; }
            else ok = parse_pos(r, (size_t)(dash - r), 1, &lo) && parse_pos(dash + 1, (size_t)(end - dash - 1), 1, &hi) && lo <= hi;
        }
        if (!ok) { snprintf(g_err, sizeof g_err, "--region: malformed item '%.*s' (CHROM, CHROM:POS or CHROM:START-END, START <= END)", (int)(n < 200 ? n : 200), p); return HPGV_ERR_INVALID; }
        if (reg_add(R, p, cl, lo, hi)) { snprintf(g_err, sizeof g_err, "out of memory for the regions"); return HPGV_ERR_NOMEM; }
        if (!e) break;
        p = e + 1;
    }
    reg_finish(R);
    return HPGV_OK;
}

/* --region-file: GFF rows (tab-separated; blank and '#' lines skipped): column 1 the sequence, 3 the feature, 4 and 5 the
 * bounds; with a type, only the rows of that feature.  Every row is checked, whatever its feature */
static int parse_gff(const char *path, const char *type, reg_set_t *R) {
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(g_err, sizeof g_err, "--region-file: cannot open %s: %s", path, strerror(errno)); return HPGV_ERR_INVALID; }
    char *line = NULL;
    size_t cap = 0;
    ssize_t len;
    long row = 0;
    int rc = HPGV_OK;
    while (!rc && (len = getline(&line, &cap, f)) >= 0) {
        row++;
        while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
        if (len == 0 || line[0] == '#') continue;
        const char *col[5];
        size_t cl[5];
        int nc = 0;
        const char *p = line;
        while (nc < 5) {
            const char *t = strchr(p, '\t');
            col[nc] = p; cl[nc] = t ? (size_t)(t - p) : strlen(p); nc++;
            if (!t) break;
            p = t + 1;
        }
        long lo, hi;
        if (nc < 5 || cl[0] == 0 || !parse_pos(col[3], cl[3], 1, &lo) || !parse_pos(col[4], cl[4], 1, &hi) || lo > hi) {
            snprintf(g_err, sizeof g_err, "--region-file: row %ld of %s is not a GFF row (sequence, source, feature, start <= end, ...)", row, path);
            rc = HPGV_ERR_INVALID;
            break;
        }
        if (type && (strlen(type) != cl[2] || memcmp(type, col[2], cl[2]))) continue;
        if (reg_add(R, col[0], cl[0], lo, hi)) { snprintf(g_err, sizeof g_err, "out of memory for the regions"); rc = HPGV_ERR_NOMEM; }
    }
    if (!rc && ferror(f)) { snprintf(g_err, sizeof g_err, "--region-file: cannot read %s", path); rc = HPGV_ERR_INVALID; }
    free(line);
    fclose(f);
    if (!rc) reg_finish(R);
    return rc;
}

/* ---- the parsed setting, shared by the runs that started under it ---- */
struct rec_filters {
    hpgv_run_record_filters_t f;                         /* strings: the copies below */
    char *regions, *region_file, *region_type;
    reg_set_t reg, reg_file;
    int refs;
};

static pthread_mutex_t g_rec_mu = PTHREAD_MUTEX_INITIALIZER;
static rec_filters_t *g_rec;                             /* NULL: all off */

static void rec_free(rec_filters_t *r) {
    if (!r) return;
    free(r->regions); free(r->region_file); free(r->region_type);
    reg_free(&r->reg); reg_free(&r->reg_file);
    free(r);
}

rec_filters_t *rec_filters_take(void) {
    pthread_mutex_lock(&g_rec_mu);
    rec_filters_t *r = g_rec;
    if (r) r->refs++;
    pthread_mutex_unlock(&g_rec_mu);
    return r;
}
void rec_filters_put(rec_filters_t *r) {
    if (!r) return;
    pthread_mutex_lock(&g_rec_mu);
    const int last = --r->refs == 0;
    pthread_mutex_unlock(&g_rec_mu);
    if (last) rec_free(r);
}
const hpgv_run_record_filters_t *rec_filters_of(const rec_filters_t *r) { return r ? &r->f : NULL; }
int rec_filters_inheritance(const rec_filters_t *r) { return r && (r->f.min_dominant >= 0.0 || r->f.min_recessive >= 0.0); }

int hpgv_run_set_record_filters(const hpgv_run_record_filters_t *f) {
    rec_filters_t *r = NULL;
    if (f) {
        const int active = f->min_coverage >= 0 || f->regions || f->region_file || f->snp >= 0 || f->var_type >= 0 || f->indel >= 0 ||
                           f->min_dominant >= 0.0 || f->min_recessive >= 0.0;
        if (f->snp < -1 || f->snp > 1) { snprintf(g_err, sizeof g_err, "--snp is -1 (off), 0 (exclude) or 1 (include), not %d", f->snp); return HPGV_ERR_INVALID; }
        if (f->indel < -1 || f->indel > 1) { snprintf(g_err, sizeof g_err, "--indel is -1 (off), 0 (exclude) or 1 (include), not %d", f->indel); return HPGV_ERR_INVALID; }
        if (f->var_type != -1 && f->var_type != HPGV_VAR_SNV && f->var_type != HPGV_VAR_INDEL && f->var_type != HPGV_VAR_STRUCTURAL) {
            snprintf(g_err, sizeof g_err, "--var-type is -1 (off) or HPGV_VAR_SNV / _INDEL / _STRUCTURAL, not %d", f->var_type); return HPGV_ERR_INVALID;
        }
        if (!(f->min_dominant <= 1.0) || !(f->min_recessive <= 1.0)) { snprintf(g_err, sizeof g_err, "the --inh-dom / --inh-rec thresholds are at most 1"); return HPGV_ERR_INVALID; }
        if (f->region_type && !f->region_file) { snprintf(g_err, sizeof g_err, "--region-type needs --region-file"); return HPGV_ERR_INVALID; }
        if (active) {
            if (!(r = (rec_filters_t *)calloc(1, sizeof *r))) { snprintf(g_err, sizeof g_err, "out of memory for the record filters"); return HPGV_ERR_NOMEM; }
            r->f = *f;
            if (r->f.min_dominant < 0.0) r->f.min_dominant = -1.0;
            if (r->f.min_recessive < 0.0) r->f.min_recessive = -1.0;
            int rc = HPGV_OK;
            if ((f->regions && !(r->regions = strdup(f->regions))) || (f->region_file && !(r->region_file = strdup(f->region_file))) ||
                (f->region_type && !(r->region_type = strdup(f->region_type)))) { snprintf(g_err, sizeof g_err, "out of memory for the record filters"); rc = HPGV_ERR_NOMEM; }
            if (!rc && r->regions) rc = parse_regions(r->regions, &r->reg);
            if (!rc && r->region_file) rc = parse_gff(r->region_file, r->region_type, &r->reg_file);
            if (rc) { rec_free(r); return rc; }
            r->f.regions = r->regions; r->f.region_file = r->region_file; r->f.region_type = r->region_type;
            r->refs = 1;
        }
    }
    pthread_mutex_lock(&g_rec_mu);
    rec_filters_t *old = g_rec;
    g_rec = r;
    pthread_mutex_unlock(&g_rec_mu);
    rec_filters_put(old);
    return HPGV_OK;
}

/* ---- the verdict of one record ---- */
/* the variant type of a record from REF's length and ALT (hpgv_host.h): HPGV_VAR_* or 0 (an MNP, ALT '.': none of the three) */
static int var_type_of(int lr, const char *alt, int la) {
    if (la <= 0 || (la == 1 && alt[0] == '.')) return 0;
    int structural = 0, snv = lr == 1, len_diff = 0;
    for (int k = 0, start = 0; k <= la; k++) {
        if (k < la && alt[k] != ',') continue;
        const int n = k - start;
        const char *a = alt + start;
        if (n > 0 && a[0] == '<') structural = 1;
        if (memchr(a, '[', (size_t)n) || memchr(a, ']', (size_t)n)) structural = 1;
        if (n != 1 || a[0] == '.') snv = 0;
        if (n != lr) len_diff = 1;
        start = k + 1;
    }
    if (structural) return HPGV_VAR_STRUCTURAL;
    if (snv) return HPGV_VAR_SNV;
    return len_diff ? HPGV_VAR_INDEL : 0;
}

/* the field filters of the setting (record_passes has checked the line has CHROM .. ALT) */
int rec_filters_pass(const rec_filters_t *r, const run_batch_t *b, int i) {
    const hpgv_run_record_filters_t *F = &r->f;
    const uint32_t *fo = b->field_off + 10 * (size_t)i;
    const char *l = b->text + b->line_off[i];
    if (F->regions || F->region_file) {
        long pos;
        if (!parse_pos(l + fo[1], (size_t)(fo[2] - 1 - fo[1]), 0, &pos)) return 0;
        const size_t cl = (size_t)(fo[1] - 1 - fo[0]);
        if (F->regions && !reg_has(&r->reg, l + fo[0], cl, pos)) return 0;
        if (F->region_file && !reg_has(&r->reg_file, l + fo[0], cl, pos)) return 0;
    }
    if (F->min_coverage >= 0) {
        const char *info; size_t n; long long dp;
        if (!record_info(b, i, &info, &n) || !info_dp(info, n, &dp) || dp < (long long)F->min_coverage) return 0;
    }
    if (F->snp >= 0) {
        const int dot = fo[3] - 1 - fo[2] == 1 && l[fo[2]] == '.';
        if (F->snp == 1 ? dot : !dot) return 0;
    }
    if (F->var_type >= 0 || F->indel >= 0) {
        const int t = var_type_of((int)(fo[4] - 1 - fo[3]), l + fo[4], (int)(fo[5] - 1 - fo[4]));
        if (F->var_type >= 0 && t != F->var_type) return 0;
        if (F->indel >= 0 && (t == HPGV_VAR_INDEL) != (F->indel == 1)) return 0;
    }
    return 1;
}

/* ---- the ##FILTER lines of the filter tool (after the five of hpgv_run_filters_t) ---- */
static void put_escaped(FILE *f, const char *s) {
    for (; *s; s++) { if (*s == '"' || *s == '\\') putc('\\', f); putc(*s, f); }
}
void rec_filters_header(FILE *f, const rec_filters_t *r) {
    if (!r) return;
    const hpgv_run_record_filters_t *F = &r->f;
    static const char *types[] = { "", "snv", "indel", "structural" };
    if (F->min_coverage >= 0) fprintf(f, "##FILTER=<ID=coverage,Description=\"Coverage >= %ld\">\n", F->min_coverage);
    if (F->regions) { fputs("##FILTER=<ID=region,Description=\"Regions ", f); put_escaped(f, F->regions); fputs("\">\n", f); }
    if (F->region_file) {
        fputs("##FILTER=<ID=region-file,Description=\"Regions of file ", f); put_escaped(f, F->region_file);
        if (F->region_type) { fputs(" of type ", f); put_escaped(f, F->region_type); }
        fputs("\">\n", f);
    }
    if (F->snp >= 0) fprintf(f, "##FILTER=<ID=snp,Description=\"SNP %s\">\n", F->snp ? "include" : "exclude");
    if (F->var_type >= 0) fprintf(f, "##FILTER=<ID=var-type,Description=\"Variant type == %s\">\n", types[F->var_type]);
    if (F->indel >= 0) fprintf(f, "##FILTER=<ID=indel,Description=\"Indels %s\">\n", F->indel ? "include" : "exclude");
    if (F->min_dominant >= 0.0) fprintf(f, "##FILTER=<ID=inh-dom,Description=\"Samples following a dominant inheritance pattern >= %g\">\n", F->min_dominant);
    if (F->min_recessive >= 0.0) fprintf(f, "##FILTER=<ID=inh-rec,Description=\"Samples following a recessive inheritance pattern >= %g\">\n", F->min_recessive);
}
