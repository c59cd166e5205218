/* host_vcftools.c -- the VCF tools' batch steps and writers: filter and split.
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"
#include <limits.h>

/* ---- HPGV_OUT_BGZF: the filter and split tools' files as bgzip.  The records are deflated on the device that holds them
 *      (hpgv_text_partition_bgzf, hpgv_text_multisplit_bgzf); what the host adds -- headers, a missing last newline, a batch
 *      whose empty lines must be taken out first -- goes through zlib, in whole members of at most 65 280 text bytes ---- */
static int g_out_mode = HPGV_OUT_PLAIN;
int hpgv_run_set_output_compression(int mode) {
    if (mode != HPGV_OUT_PLAIN && mode != HPGV_OUT_BGZF) { snprintf(g_err, sizeof g_err, "unknown output compression %d", mode); return HPGV_ERR_INVALID; }
    g_out_mode = mode;
    return HPGV_OK;
}
int out_compression_now(void) { return g_out_mode; }
/* bgzip members never outgrow the text by more than 31 bytes per block; split: a batch's ranges have 255 buckets each */
size_t out_batch_cap(const run_t *R, size_t batch_bytes) {
    return R->out_bgzf ? hpgv_bgzf_deflate_bound(batch_bytes, R->tool == RUN_SPLIT ? 256 : 2) : batch_bytes;
}

int bgzf_write_eof(FILE *f) {
    static const unsigned char eof[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    return fwrite(eof, 1, sizeof eof, f) != sizeof eof;
}
enum { BGZF_TEXT = HPGV_BGZF_BLOCK_TEXT, BGZF_MEMBER = 65536 };
/* n bytes of text as members; level 0 (stored) when the deflated block would not fit a member */
static int bgzf_write_text(FILE *f, const char *p, size_t n) {
    unsigned char *m = (unsigned char *)malloc(BGZF_MEMBER);
    if (!m) return 1;
    int bad = 0;
    for (size_t at = 0; at < n && !bad; at += BGZF_TEXT) {
        const size_t len = n - at < BGZF_TEXT ? n - at : BGZF_TEXT;
        size_t pay = 0;
        for (int level = Z_DEFAULT_COMPRESSION, done = 0; !done && !bad; level = 0) {
            z_stream z;
            memset(&z, 0, sizeof z);
            if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { bad = 1; break; }
            z.next_in = (Bytef *)(p + at); z.avail_in = (uInt)len;
            z.next_out = m + 18; z.avail_out = BGZF_MEMBER - 26;
            done = deflate(&z, Z_FINISH) == Z_STREAM_END;
            pay = z.total_out;
            deflateEnd(&z);
            if (!done && level == 0) bad = 1;
        }
        if (bad) break;
        static const unsigned char head[16] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0 };
        memcpy(m, head, 16);
        const uint32_t bsize = (uint32_t)pay + 25, crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(p + at), (uInt)len), isize = (uint32_t)len;
        m[16] = (unsigned char)bsize; m[17] = (unsigned char)(bsize >> 8);
        for (int k = 0; k < 4; k++) { m[18 + pay + k] = (unsigned char)(crc >> (8 * k)); m[22 + pay + k] = (unsigned char)(isize >> (8 * k)); }
        bad = fwrite(m, 1, pay + 26, f) != pay + 26;
    }
    free(m);
    return bad;
}

static int keep_reserve(run_batch_t *b, int n) {      /* room in b->keep for a byte per line */
    if (b->keep_cap >= n) return HPGV_OK;
    free(b->keep);
    b->keep_cap = (b->keep = (uint8_t *)malloc((size_t)n + 1)) ? n : 0;
    return b->keep ? HPGV_OK : HPGV_ERR_NOMEM;
}

/* the filter tool's engine step after hpgv_filter_text, while the batch's text is still on the device: the verdict of every
 * line (record_passes: the heads are enough), then the lines partitioned there into the batch's own page-locked buffer --
 * the kept lines first, then the others, both in file order */
int filter_partition(run_batch_t *b) {
    const int n = b->n_lines;
    if (n > b->max_lines) return HPGV_ERR_UNSUPPORTED;                /* (hpgv_filter_text kept nothing then) */
    b->n_pass = b->n_rej = 0; b->n_blank = 0; b->part_kept = b->part_total = 0;
    if (keep_reserve(b, n)) { (void)hpgv_text_partition(g_ctx, b->text, NULL, 0, NULL, 0, NULL, NULL); return HPGV_ERR_NOMEM; }
    for (int i = 0; i < n; i++) {
        const int k = record_passes(b, i);
        b->keep[i] = (uint8_t)k;
        if (k) b->n_pass++;
        else if (b->line_off[i + 1] - b->line_off[i] == 1 && b->text[b->line_off[i]] == '\n') b->n_blank++;      /* an empty line */
        else b->n_rej++;
    }
    uint64_t kept = 0, total = 0;
    const run_t *R = b->run;
    /* bgzip output: both parts deflated where they lie.  A batch with empty lines among the rejected ones comes back as text:
     * the writer takes them out first (write_region) and deflates on the host */
    b->part_bgzf = R->out_bgzf && !(R->save_rejected && b->n_blank > 0);
    if (b->part_bgzf) {
        uint64_t comp[2] = {0, 0};
        const int rc = hpgv_text_partition_bgzf(g_ctx, b->text, b->keep, n, (uint8_t *)b->text, b->text_cap, R->save_rejected, &kept, &total, comp, b->part_last);
        b->part_kept = comp[0]; b->part_total = comp[0] + comp[1];
        return rc;
    }
    const int rc = hpgv_text_partition(g_ctx, b->text, b->keep, n, b->text, b->text_cap, &kept, &total);
    b->part_kept = kept; b->part_total = total;
    return rc;
}

/* ---- hpg-var-vcf split (split.c:37-122, split_runner.c:23-190): every record to a file picked by its CHROM or its DP ---- */
enum { SPLIT_RANGE_BUCKETS = 255, SPLIT_NO_FILE = 255 };

static inline unsigned char ascii_lower(unsigned char c) { return c >= 'A' && c <= 'Z' ? (unsigned char)(c | 0x20) : c; }
static uint64_t hash_icase(const char *p, size_t n) {   /* FNV-1a of the lower-cased bytes: the key of cp_hash_istring */
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < n; k++) h = (h ^ ascii_lower((unsigned char)p[k])) * 1099511628211ull;
    return h;
}
static int eq_icase(const char *a, size_t na, const char *b, size_t nb) {
    if (na != nb) return 0;
    for (size_t k = 0; k < na; k++) if (ascii_lower((unsigned char)a[k]) != ascii_lower((unsigned char)b[k])) return 0;
    return 1;
}

/* the split name of coverage bucket j (0 .. n_iv: the intervals, n_iv + 1: no DP) */
static int coverage_name(char *out, size_t cap, const run_t *R, int j) {
    const long *iv = R->iv; const int n = R->n_iv;
    if (j > n) return snprintf(out, cap, "coverage_missing");
    if (j == n) return snprintf(out, cap, "coverage_%ld_N", iv[n - 1]);
    return snprintf(out, cap, "coverage_%ld_%ld", j ? iv[j - 1] : 0L, iv[j]);
}

/* a bucket named pre || body */
static int sp_add_bucket(run_batch_t *b, const char *pre, size_t npre, const char *body, size_t nbody) {
    if (b->sp_n_buckets == b->sp_bucket_cap) {
        const int c = b->sp_bucket_cap ? 2 * b->sp_bucket_cap : 256;
        uint64_t *l = (uint64_t *)realloc(b->sp_len, sizeof(uint64_t) * (size_t)c);
        if (l) b->sp_len = l;
        int *nm = (int *)realloc(b->sp_name, sizeof(int) * (size_t)c);
        if (nm) b->sp_name = nm;
        if (!l || !nm) return HPGV_ERR_NOMEM;
        b->sp_bucket_cap = c;
    }
    const size_t len = npre + nbody;
    if (b->sp_names_len + len + 1 > b->sp_names_cap) {
        const size_t c = 2 * (b->sp_names_len + len + 1) + 4096;
        char *p = c > (size_t)INT32_MAX ? NULL : (char *)realloc(b->sp_names, c);
        if (!p) return HPGV_ERR_NOMEM;
        b->sp_names = p; b->sp_names_cap = c;
    }
    b->sp_name[b->sp_n_buckets] = (int)b->sp_names_len;
    b->sp_len[b->sp_n_buckets++] = 0;
    memcpy(b->sp_names + b->sp_names_len, pre, npre);
    memcpy(b->sp_names + b->sp_names_len + npre, body, nbody);
    b->sp_names[b->sp_names_len + len] = 0;
    b->sp_names_len += len + 1;
    return HPGV_OK;
}
static int sp_add_range(run_batch_t *b, int first, int n, int nb) {
    if (b->sp_n_ranges == b->sp_range_cap) {
        const int c = b->sp_range_cap ? 2 * b->sp_range_cap : 16;
        int *r = (int *)realloc(b->sp_range, sizeof(int) * 3 * (size_t)c);
        if (!r) return HPGV_ERR_NOMEM;
        b->sp_range = r; b->sp_range_cap = c;
    }
    int *r = b->sp_range + 3 * b->sp_n_ranges++;
    r[0] = first; r[1] = n; r[2] = nb;
    return HPGV_OK;
}

/* the bucket of every line, from the heads (CHROM and INFO are in them whatever the text's residence); a batch with more than
 * SPLIT_RANGE_BUCKETS split names is cut into consecutive line ranges of at most that many.  A line with the CHROM of the line
 * before it takes its bucket without a lookup. */
static int split_keys(run_batch_t *b) {
    const run_t *R = b->run;
    const int n = b->n_lines;
    int tab[512];                                         /* open addressing over the range's buckets (<= 255): bucket + 1 */
    size_t tab_len[SPLIT_RANGE_BUCKETS];                  /* chromosome: the CHROM length of each bucket of the range */
    int *cov = (int *)malloc(sizeof(int) * ((size_t)R->n_iv + 2));      /* coverage: bucket of interval j in the range, or -1 */
    char name[96];
    if (!cov) return HPGV_ERR_NOMEM;
    memset(tab, 0, sizeof tab);
    for (int j = 0; j < R->n_iv + 2; j++) cov[j] = -1;
    int first = 0, nb = 0, base = 0, prev = -1, rc = HPGV_OK;           /* base: global index of the range's bucket 0 */
    const char *pc = NULL; size_t pl = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t *fo = b->field_off + 10 * (size_t)i;
        if (fo[7] == 0xFFFFFFFFu) { b->keep[i] = SPLIT_NO_FILE; b->n_skip++; continue; }     /* fewer than CHROM .. INFO, or empty */
        const char *l = b->text + b->line_off[i];
        int id = -1, j = 0;
        const char *c = l; const size_t cl = fo[1] - 1;
        uint64_t h = 0;
        if (R->criterion == HPGV_SPLIT_CHROMOSOME) {
            if (prev >= 0 && cl == pl && !memcmp(c, pc, cl)) id = prev;
            else {
                h = hash_icase(c, cl);
                for (size_t s = h & 511; tab[s]; s = (s + 1) & 511) {
                    const int t = tab[s] - 1;
                    if (eq_icase(c, cl, b->sp_names + b->sp_name[base + t] + 11, tab_len[t])) { id = t; break; }
                }
            }
        } else {
            const char *info; size_t ni;
            long long v = 0;
            if (!record_info(b, i, &info, &ni) || !info_dp(info, ni, &v)) j = R->n_iv + 1;
            else {                                        /* the first bound >= v, or n_iv */
                int lo = 0, hi = R->n_iv;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (v > (long long)R->iv[mid]) lo = mid + 1; else hi = mid; }
                j = lo;
            }
            id = cov[j];
        }
        if (id < 0) {                                     /* a split name new to the range */
            if (nb == SPLIT_RANGE_BUCKETS) {
                if (sp_add_range(b, first, i - first, nb)) { rc = HPGV_ERR_NOMEM; break; }
                first = i; base += nb; nb = 0; prev = -1;
                memset(tab, 0, sizeof tab);
                for (int k = 0; k < R->n_iv + 2; k++) cov[k] = -1;
            }
            id = nb++;
            if (R->criterion == HPGV_SPLIT_CHROMOSOME) {
                size_t t = h & 511;
                while (tab[t]) t = (t + 1) & 511;
                tab[t] = id + 1; tab_len[id] = cl;
                if (sp_add_bucket(b, "chromosome_", 11, c, cl)) { rc = HPGV_ERR_NOMEM; break; }
            } else {
                cov[j] = id;
                const int len = coverage_name(name, sizeof name, R, j);
                if (sp_add_bucket(b, name, (size_t)len, "", 0)) { rc = HPGV_ERR_NOMEM; break; }
            }
        }
        b->keep[i] = (uint8_t)id; b->n_pass++;
        prev = id; pc = c; pl = cl;
    }
    if (!rc && nb > 0 && sp_add_range(b, first, n - first, nb)) rc = HPGV_ERR_NOMEM;
    free(cov);
    return rc;
}

/* the split tool's engine step after hpgv_filter_text, while the batch's text is still on the device: the bucket of every
 * line, then each line range split there into the next part of the batch's own page-locked buffer */
int split_partition(run_batch_t *b) {
    const int n = b->n_lines;
    if (n > b->max_lines) return HPGV_ERR_UNSUPPORTED;
    b->n_pass = 0; b->n_skip = 0; b->sp_n_ranges = 0; b->sp_n_buckets = 0; b->sp_names_len = 0;
    int rc = keep_reserve(b, n);
    const double t0 = now_s();
    if (!rc) rc = split_keys(b);                           /* every key before the first copy back overwrites the heads */
    __atomic_add_fetch(&b->run->key_ns, (long)((now_s() - t0) * 1e9), __ATOMIC_RELAXED);
    uint64_t boff[SPLIT_RANGE_BUCKETS + 1];
    size_t pos = 0;
    for (int r = 0, k = 0; !rc && r < b->sp_n_ranges; r++) {
        const int *R = b->sp_range + 3 * r;
        uint8_t last[SPLIT_RANGE_BUCKETS];
        /* bgzip output: the buckets deflated where they lie; a range whose members do not fit the buffer's rest comes back as
         * text, which the writer deflates on the host */
        int members = b->run->out_bgzf;
        if (members && hpgv_text_multisplit_bgzf(g_ctx, b->text, b->keep + R[0], R[0], R[1], R[2], (uint8_t *)b->text + pos, b->text_cap - pos, boff, last)) members = 0;
        if (!members) rc = hpgv_text_multisplit(g_ctx, b->text, b->keep + R[0], R[0], R[1], R[2], b->text + pos, b->text_cap - pos, boff);
        if (rc) break;
        for (int j = 0; j < R[2]; j++) b->sp_len[k++] = (boff[j + 1] - boff[j]) | (members ? SP_MEMBERS | (last[j] != '\n' ? SP_NEEDS_NL : 0) : 0);
        pos += (size_t)boff[R[2]];
    }
    (void)hpgv_text_partition(g_ctx, b->text, NULL, 0, NULL, 0, NULL, NULL);     /* the hold released */
    return rc;
}

/* hpg-var-vcf filter: the lines of one batch in its two files.  The kept region holds no empty line; the rejected one
 * holds n_blank of them, each a '\n' at the region's start or right behind another '\n', and they go to neither file.  The
 * file's last line may lack its newline: it gets one. */
typedef struct { FILE *f; char *buf; size_t len; } region_sink_t;       /* to the file, or (buf != NULL) gathered for the host's deflate */
static int sink_put(region_sink_t *s, const char *p, size_t n) {
    if (s->buf) { memcpy(s->buf + s->len, p, n); s->len += n; return 0; }
    return fwrite(p, 1, n, s->f) != n;
}
static int region_put(region_sink_t *s, const char *p, size_t n, int blanks) {
    size_t i = 0;
    while (blanks > 0 && i < n) {
        if (p[i] == '\n') { i++; blanks--; continue; }
        const char *q = (const char *)memmem(p + i, n - i, "\n\n", 2);
        const size_t e = q ? (size_t)(q - p) + 1 : n;
        if (sink_put(s, p + i, e - i)) return 1;
        i = e;
    }
    if (i < n && sink_put(s, p + i, n - i)) return 1;
    if (n && p[n - 1] != '\n' && sink_put(s, "\n", 1)) return 1;
    return 0;
}
static int write_region(FILE *f, const char *p, size_t n, int blanks) {
    region_sink_t s = { f, NULL, 0 };
    return region_put(&s, p, n, blanks);
}
/* the same bytes as BGZF members, deflated on the host */
static int write_region_bgzf(FILE *f, const char *p, size_t n, int blanks) {
    region_sink_t s = { f, (char *)malloc(n + 1), 0 };
    if (!s.buf) return 1;
    const int bad = region_put(&s, p, n, blanks) || bgzf_write_text(f, s.buf, s.len);
    free(s.buf);
    return bad;
}
/* members the device made, and the newline their text's last line lacks */
static int write_members(FILE *f, const char *p, size_t n, int needs_nl) {
    if (n && fwrite(p, 1, n, f) != n) return 1;
    return needs_nl && bgzf_write_text(f, "\n", 1);
}
int write_filter_batch(FILE *kept, FILE *rejected, const run_batch_t *b) {
    const size_t nk = (size_t)b->part_kept, nr = (size_t)(b->part_total - b->part_kept);
    if (b->part_bgzf)
        return write_members(kept, b->text, nk, b->part_last[0] != '\n') || (rejected && write_members(rejected, b->text + nk, nr, b->part_last[1] != '\n'));
    if (b->run->out_bgzf)
        return write_region_bgzf(kept, b->text, nk, 0) || (rejected && write_region_bgzf(rejected, b->text + nk, nr, b->n_blank));
    if (write_region(kept, b->text, nk, 0)) return 1;
    return rejected && write_region(rejected, b->text + nk, nr, b->n_blank);
}
/* the header of both files (filter_runner.c:129-137): the input's meta lines, one ##FILTER line per active filter, #CHROM */
static int filter_header_text(FILE *f, const run_t *R);
int write_filter_header(FILE *f, const run_t *R) {
    if (!R->out_bgzf) return filter_header_text(f, R);
    char *buf = NULL; size_t len = 0;                     /* the same text, as members */
    FILE *mem = open_memstream(&buf, &len);
    if (!mem) return 1;
    int bad = filter_header_text(mem, R);
    bad = fclose(mem) != 0 || bad;
    if (!bad) bad = bgzf_write_text(f, buf, len);
    free(buf);
    return bad;
}
static int filter_header_text(FILE *f, const run_t *R) {
    const hpgv_run_filters_t *F = &R->filters;
    if (R->chrom_off && fwrite(R->hdr, 1, R->chrom_off, f) != R->chrom_off) return 1;
    if (F->min_maf >= 0.0) fprintf(f, "##FILTER=<ID=maf,Description=\"Minor allele frequency >= %g\">\n", F->min_maf);
    if (F->max_missing >= 0.0) fprintf(f, "##FILTER=<ID=missing,Description=\"Rate of missing genotypes <= %g\">\n", F->max_missing);
    if (F->max_mendel_errors >= 0) fprintf(f, "##FILTER=<ID=mendel,Description=\"Mendelian errors <= %g\">\n", (double)F->max_mendel_errors);
    if (F->num_alleles >= 0) fprintf(f, "##FILTER=<ID=alleles,Description=\"Number of alleles == %g\">\n", (double)F->num_alleles);
    if (F->min_quality >= 0.0) fprintf(f, "##FILTER=<ID=quality,Description=\"Quality >= %g\">\n", F->min_quality);
    rec_filters_header(f, R->rf);
    return R->rd.chrom_len && fwrite(R->rd.chrom_line, 1, R->rd.chrom_len, f) != R->rd.chrom_len;
}

/* hpg-var-vcf split: the output files, by split name (case-insensitive, as the reference's cp_hash_istring table).  A file is
 * created by the first record it receives, with the input header, and named after that record; at most SPLIT_OPEN_MAX are
 * open at once -- the least recently written is closed and reopened later for appending. */

static FILE *split_file(run_t *R, const char *name) {
    split_files_t *S = &R->SF;
    snprintf(g_err, sizeof g_err, "out of memory for the split files");
    const size_t nl = strlen(name);
    if (nl + 1 > S->key_cap) { char *k = (char *)realloc(S->key, 2 * nl + 64); if (!k) return NULL; S->key = k; S->key_cap = 2 * nl + 64; }
    for (size_t q = 0; q <= nl; q++) S->key[q] = (char)ascii_lower((unsigned char)name[q]);
    if (!S->ids && !(S->ids = sample_ids_new(256))) return NULL;
    int k = sample_ids_get(S->ids, S->key);
    if (k < 0) {                                         /* a new file: <out_dir>/<split name, '/' and '%' escaped>_<base> */
        if (S->n == S->cap) {
            const int c = S->cap ? 2 * S->cap : 64;
            split_file_t *f = (split_file_t *)realloc(S->f, sizeof *f * (size_t)c);
            if (!f) return NULL;
            S->f = f; S->cap = c;
        }
        split_file_t *F = &S->f[S->n];
        memset(F, 0, sizeof *F);
        const char *dir = R->dir, *base = R->base;
        const size_t dl = strlen(dir), bl = strlen(base);
        F->name = dupn(S->key, (int)nl);                 /* the table's key */
        F->path = (char *)malloc(dl + 3 * nl + bl + 3 + 3);
        if (!F->name || !F->path) { free(F->name); free(F->path); return NULL; }
        char *p = F->path;
        memcpy(p, dir, dl); p += dl; *p++ = '/';
        for (size_t q = 0; q < nl; q++) {
            if (name[q] == '/') { memcpy(p, "%2F", 3); p += 3; }
            else if (name[q] == '%') { memcpy(p, "%25", 3); p += 3; }
            else *p++ = name[q];
        }
        *p++ = '_'; memcpy(p, base, bl + 1);
        if (R->out_bgzf) memcpy(p + bl, ".gz", 4);
        if (!sample_ids_put(S->ids, F->name, S->n)) { free(F->name); free(F->path); return NULL; }
        k = S->n++;
    }
    split_file_t *F = &S->f[k];
    F->last = ++S->clock;
    if (F->fd) return F->fd;
    if (S->n_open == SPLIT_OPEN_MAX) {                   /* close the least recently written */
        int o = 0;
        for (int q = 1; q < S->n_open; q++) if (S->f[S->open[q]].last < S->f[S->open[o]].last) o = q;
        split_file_t *G = &S->f[S->open[o]];
        const int bad = fclose(G->fd) != 0;
        G->fd = NULL;
        S->open[o] = S->open[--S->n_open];
        if (bad) { snprintf(g_err, sizeof g_err, "cannot write %s", G->path); return NULL; }
    }
    const int created = !F->created;
    F->fd = fopen(F->path, created ? "wb" : "ab");       /* only the first open in a run truncates */
    if (!F->fd) { snprintf(g_err, sizeof g_err, "cannot create %s", F->path); return NULL; }
    S->open[S->n_open++] = k;
    if (created) {
        F->created = 1; R->files++;
        const int bad = R->out_bgzf ? bgzf_write_text(F->fd, R->hdr, R->chrom_off) || bgzf_write_text(F->fd, R->rd.chrom_line, R->rd.chrom_len)
                                    : (R->chrom_off && fwrite(R->hdr, 1, R->chrom_off, F->fd) != R->chrom_off) ||
                                      (R->rd.chrom_len && fwrite(R->rd.chrom_line, 1, R->rd.chrom_len, F->fd) != R->rd.chrom_len);
        if (bad) { snprintf(g_err, sizeof g_err, "cannot write %s", F->path); return NULL; }
    }
    return F->fd;
}
int write_split_batch(run_t *R, const run_batch_t *b) {
    size_t pos = 0;
    for (int k = 0; k < b->sp_n_buckets; k++) {
        const char *name = b->sp_names + b->sp_name[k];
        FILE *fd = split_file(R, name);
        if (!fd) return 1;
        const size_t len = (size_t)SP_LEN(b->sp_len[k]);
        const int bad = b->sp_len[k] & SP_MEMBERS ? write_members(fd, b->text + pos, len, (b->sp_len[k] & SP_NEEDS_NL) != 0)
                      : R->out_bgzf ? write_region_bgzf(fd, b->text + pos, len, 0) : write_region(fd, b->text + pos, len, 0);
        if (bad) { snprintf(g_err, sizeof g_err, "cannot write the file of %s", name); return 1; }
        pos += len;
    }
    return 0;
}
/* bgzf: every file ends with the EOF block, written here once -- a file closed under the open-files rule is opened again */
int split_files_close(split_files_t *S, int bgzf) {
    int bad = 0;
    for (int k = 0; k < S->n; k++) {
        if (bgzf && !S->f[k].fd && S->f[k].created) S->f[k].fd = fopen(S->f[k].path, "ab");
        if (bgzf && (!S->f[k].fd || bgzf_write_eof(S->f[k].fd)) && !bad) { bad = 1; snprintf(g_err, sizeof g_err, "cannot write %s", S->f[k].path); }
        if (S->f[k].fd && fclose(S->f[k].fd) != 0 && !bad) { bad = 1; snprintf(g_err, sizeof g_err, "cannot write %s", S->f[k].path); }
        free(S->f[k].name); free(S->f[k].path);
    }
    free(S->f); free(S->key); sample_ids_free(S->ids);
    memset(S, 0, sizeof *S);
    return bad;
}
