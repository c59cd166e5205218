/* host_bgzf.c -- a bgzip file staged on the device(s): upload, block table, decode, CRC check, in parts over a group.
 * One uploader, one stager and one publisher per file (or part); the stager takes the block table's rows from the device
 * scan of the uploaded bytes or, where the text's size must be known first, from the table the host has walked.
 * Part of libhpgv_host.so (see hpgv_host_internal.h for the map of its units). */
#include "hpgv_host_internal.h"

/* the tokenizer's tile records of a text of about `bytes` bytes that the device is going to decode and check: zeroed device
 * memory (hpgv.h "hpgv_bgzf_verify_tiles_dev").  Not having them only means the windows are tokenized the ordinary way. */
static void tiles_alloc(source_t *s, size_t bytes) {
    s->d_tiles = NULL; s->n_tiles = 0; s->d_tiles_cap = 0;
    if (!g_env.bgzf_verify || g_env.no_decode_tiles) return;
    const size_t nb = hpgv_text_tiles_bytes((uint64_t)bytes);
    size_t cap = 0;
    void *p = dev_tiles_get(nb, &cap);
    if (!p) return;
    if (hpgv_memset_dev(CTX, p, 0, nb, NULL) != HPGV_OK) { dev_tiles_put(p, cap); return; }
    s->d_tiles = p; s->n_tiles = nb / 32 - 1; s->d_tiles_cap = cap;
}
static void tiles_free(source_t *s) { if (s->d_tiles) { dev_tiles_put(s->d_tiles, s->d_tiles_cap); s->d_tiles = NULL; s->n_tiles = 0; s->d_tiles_cap = 0; } }
static size_t pread_full(int fd, void *buf, size_t n, size_t pos) {
    size_t have = 0;
    while (have < n) {
        const ssize_t got = pread(fd, (char *)buf + have, n - have, (off_t)(pos + have));
        if (got <= 0) break;
        have += (size_t)got;
    }
    return have;
}

/* BGZF on the GPU: the file's blocks are decoded on the device (one lane per block, tens of thousands of blocks per launch;
 * 8 GB of VCF text in 0.1 s) and the text stays in device memory.  The reader copies it out window by window for the result
 * writers and the engine tokenizes the device copy in place (hpgv_text_alias) -- the compressed bytes are all that goes up
 * the bus, read from the file with pread into a page-locked buffer (the mapping is not touched: faulting a gigabyte in and
 * unmapping it costs more than the decoding).  A stager thread decodes the file in stretches as its bytes arrive: a short
 * one first, decoded alone, so that the header reader and the pipeline start after the time one block takes; then longer
 * ones, several launches side by side on streams of their own.  A block the device decoder refuses is decoded by the host
 * and patched in.  No memory, a file of more than 48 GB of text or fewer than 256 blocks leave the CPU path in charge.
 * HPGV_NO_GPU_INFLATE=1 switches it off. */
/* The upload: out of pageable memory a copy runs at a fifth of the bus rate, so the file goes through a page-locked ring
 * (pread, not the mapping: faulting a gigabyte in and unmapping it again costs ~90 ms).  Readers take the file's 4 MB
 * segments in turn and fill the ring's slots; the uploader copies the slots up in file order and announces every segment
 * that has arrived (s->up_done, under g_mu).  Nobody waits at a barrier: a reader waits only for its slot to be free, the
 * copier only for the next segment to be filled.  (Halves of a buffer filled by a team, with a barrier per half, left
 * the bus at 18 - 28 GB/s beside the pipeline's own threads.) */
enum { UP_SEG_DEFAULT = 4 << 20, UP_SLOTS = 16, UP_READERS_MAX = 12, UP_INFLIGHT = 2 };
static size_t g_up_seg = UP_SEG_DEFAULT;                 /* bytes per segment (HPGV_UPLOAD_SEGMENT_MB: diagnosis) */
typedef struct {
    source_t *s; char *pin; size_t n_seg;
    pthread_mutex_t mu; pthread_cond_t cv;
    size_t next;                                         /* the next segment a reader takes */
    size_t copied;                                       /* segments [0, copied) are on the device: slot i % UP_SLOTS is free for segment i < copied + UP_SLOTS */
    unsigned char filled[UP_SLOTS];
    int bad, stop;
} up_ring_t;
static void *up_reader(void *v) {
    up_ring_t *r = (up_ring_t *)v;
    for (;;) {
        pthread_mutex_lock(&r->mu);
        const size_t i = r->next < r->n_seg ? r->next++ : (size_t)-1;
        while (i != (size_t)-1 && !r->stop && !r->bad && i >= r->copied + UP_SLOTS) pthread_cond_wait(&r->cv, &r->mu);
        const int quit = i == (size_t)-1 || r->stop || r->bad;
        pthread_mutex_unlock(&r->mu);
        if (quit) return NULL;
        const size_t off = i * g_up_seg, len = off + g_up_seg <= (size_t)r->s->size ? g_up_seg : (size_t)r->s->size - off;
        const int ok = pread_full(r->s->fd, r->pin + (i % UP_SLOTS) * g_up_seg, len, off + (size_t)r->s->file_off) == len;
        pthread_mutex_lock(&r->mu);
        if (ok) r->filled[i % UP_SLOTS] = 1; else r->bad = 1;
        pthread_cond_broadcast(&r->cv);
        pthread_mutex_unlock(&r->mu);
    }
}
static void *bgzf_uploader(void *v) {
    source_t *s = (source_t *)v;
    (void)SRC_CTX(s);                                               /* this thread works on the part's member device from here on */
    void *up = NULL;
    int ok = stream_get(0, &up) == HPGV_OK;
    g_up_seg = g_env.upload_segment_mb >= 1 && g_env.upload_segment_mb <= 64 ? (size_t)g_env.upload_segment_mb << 20 : (size_t)UP_SEG_DEFAULT;
    const size_t pin_cap = g_up_seg * UP_SLOTS;
    char *pin = text_buf_get(pin_cap + 1);                          /* from the runs' cache of page-locked buffers */
    up_ring_t r;
    memset(&r, 0, sizeof r);
    r.s = s; r.pin = pin; r.n_seg = ((size_t)s->size + g_up_seg - 1) / g_up_seg;
    pthread_mutex_init(&r.mu, NULL); pthread_cond_init(&r.cv, NULL);
    pthread_t th[UP_READERS_MAX];
    int n_th = 0;
    if (ok && pin) {
        int want = default_io_threads() * 3 / 4;
        if (s->is_part || s->mp) want = want / 2 > 2 ? want / 2 : 2;    /* several parts go up side by side: they share the host's threads */
        want = want < 1 ? 1 : want > UP_READERS_MAX ? UP_READERS_MAX : want;
        for (; n_th < want; n_th++) if (pthread_create(&th[n_th], NULL, up_reader, &r) != 0) break;
    }
    ok = ok && pin && n_th > 0;
    double t_wait = 0, t_copy = 0; const double t_begin = now_s();
    /* UP_INFLIGHT copies in flight: one is waited for while the others are queued or running */
    enum { UP_INFLIGHT_MAX = 8 };
    const int depth = g_env.upload_inflight >= 1 && g_env.upload_inflight <= UP_INFLIGHT_MAX ? (int)g_env.upload_inflight : UP_INFLIGHT;
    void *stq[UP_INFLIGHT_MAX] = { up };
    for (int k = 1; ok && k < depth; k++) ok = stream_get(0, &stq[k]) == HPGV_OK;
    for (size_t i = 0; ok && i < r.n_seg + (size_t)depth - 1; i++) {
        double t0 = now_s();
        if (i < r.n_seg) {
            pthread_mutex_lock(&r.mu);
            while (!r.filled[i % UP_SLOTS] && !r.bad) pthread_cond_wait(&r.cv, &r.mu);
            ok = !r.bad;
            pthread_mutex_unlock(&r.mu);
            t_wait += now_s() - t0; t0 = now_s();
            if (!ok) break;
            const size_t off = i * g_up_seg, len = off + g_up_seg <= (size_t)s->size ? g_up_seg : (size_t)s->size - off;
            ok = hpgv_memcpy_h2d_async(CTX, (char *)s->d_comp + off, pin + (i % UP_SLOTS) * g_up_seg, len, stq[i % (size_t)depth]) == HPGV_OK;
            if (!ok) break;
        }
        if (i + 1 < (size_t)depth) continue;
        const size_t j = i + 1 - (size_t)depth, off = j * g_up_seg, len = off + g_up_seg <= (size_t)s->size ? g_up_seg : (size_t)s->size - off;
        ok = hpgv_stream_sync(CTX, stq[j % (size_t)depth]) == HPGV_OK;
        t_copy += now_s() - t0;
        pthread_mutex_lock(&r.mu);
        r.filled[j % UP_SLOTS] = 0; r.copied = j + 1;
        pthread_cond_broadcast(&r.cv);
        pthread_mutex_unlock(&r.mu);
        if (!ok) break;
        if (j == 0 && g_env.run_trace) fprintf(stderr, "uploader: first segment up %.4f s after its start\n", now_s() - t_begin);
        pthread_mutex_lock(&s->g_mu);
        s->up_done = off + len;
        const int cancel = s->u_cancel;
        pthread_cond_broadcast(&s->g_cv);
        pthread_mutex_unlock(&s->g_mu);
        if (cancel) { ok = 0; break; }
    }
    for (int k = 1; k < depth; k++) if (stq[k]) { (void)hpgv_stream_sync(CTX, stq[k]); stream_put(0, stq[k]); }
    if (up) (void)hpgv_stream_sync(CTX, up);
    if (g_env.run_trace)
        fprintf(stderr, "uploader: %.1f MB in %.4f s: %.4f s waiting for the readers (%d), %.4f s in copies\n", s->size / 1e6, now_s() - t_begin, t_wait, n_th, t_copy);
    pthread_mutex_lock(&r.mu); r.stop = 1; pthread_cond_broadcast(&r.cv); pthread_mutex_unlock(&r.mu);
    for (int k = 0; k < n_th; k++) pthread_join(th[k], NULL);
    pthread_mutex_destroy(&r.mu); pthread_cond_destroy(&r.cv);
    if (pin) text_buf_put(pin, pin_cap + 1);
    stream_put(0, up);
    pthread_mutex_lock(&s->g_mu);
    if (!ok && !s->u_cancel) s->u_err = 1;
    if (!ok && s->up_done < (size_t)s->size) s->u_err = 1;
    pthread_cond_broadcast(&s->g_cv);
    pthread_mutex_unlock(&s->g_mu);
    return NULL;
}
/* The compressed bytes start going up when the file is opened, beside whatever finds the block table: the decoder needs the
 * table, the bus does not.  0 = no memory or no thread, and nothing is left behind. */
static int upload_start(source_t *s) {
    const double t0 = now_s();
    pthread_mutex_init(&s->g_mu, NULL); pthread_cond_init(&s->g_cv, NULL);
    s->g_sync = 1; s->up_done = 0; s->u_cancel = 0; s->u_err = 0;
    if (hpgv_dev_alloc(CTX, (size_t)s->size + 16, &s->d_comp) == HPGV_OK) {
        if (g_env.run_trace) fprintf(stderr, "stage: room for the compressed file at %.4f\n", now_s() - t0);
        if (pthread_create(&s->u_thread, NULL, bgzf_uploader, s) == 0) { s->u_started = 1; return 1; }
    }
    bgzf_stage_release(s);
    return 0;
}
/* calls the uploader back (it may be through already) and waits for it: d_comp can be freed after this */
void upload_cancel(source_t *s) {
    if (!s->u_started) return;
    pthread_mutex_lock(&s->g_mu); s->u_cancel = 1; pthread_mutex_unlock(&s->g_mu);
    pthread_join(s->u_thread, NULL); s->u_started = 0;
}
/* the uploader's progress: waits until at least `want` bytes are up (or all of the file); returns how many are, 0 on failure */
static size_t wait_uploaded_some(source_t *s, size_t want) {
    if (want > (size_t)s->size) want = (size_t)s->size;
    pthread_mutex_lock(&s->g_mu);
    while (s->up_done < want && !s->u_err) pthread_cond_wait(&s->g_cv, &s->g_mu);
    const size_t have = s->u_err ? 0 : s->up_done;
    pthread_mutex_unlock(&s->g_mu);
    return have;
}

/* ---- the block table: a row per block (bgzf_rows_t), built by the host for a whole file or a few blocks at a time ---- */
int bgzf_rows_reserve(bgzf_rows_t *t, size_t cap) {
    if (cap <= t->cap) return 1;
    uint64_t *a = (uint64_t *)realloc(t->in_off, cap * 8), *b = (uint64_t *)realloc(t->out_off, cap * 8);
    uint32_t *c = (uint32_t *)realloc(t->in_len, cap * 4), *d = (uint32_t *)realloc(t->out_len, cap * 4);
    if (a) t->in_off = a;
    if (b) t->out_off = b;
    if (c) t->in_len = c;
    if (d) t->out_len = d;
    if (!a || !b || !c || !d) return 0;
    t->cap = cap;
    return 1;
}
void bgzf_rows_free(bgzf_rows_t *t) {
    free(t->in_off); free(t->out_off); free(t->in_len); free(t->out_len);
    memset(t, 0, sizeof *t);
}
/* one more row: a block of `bs` bytes at file offset `pos` whose payload begins `co` bytes in; 0 = no memory */
static int bgzf_rows_add(bgzf_rows_t *t, size_t pos, size_t bs, size_t co, size_t text, size_t is) {
    if (t->n == t->cap && !bgzf_rows_reserve(t, t->cap ? 2 * t->cap : (size_t)1 << 16)) return 0;
    t->in_off[t->n] = pos + co; t->in_len[t->n] = (uint32_t)(bs - co - 8); t->out_off[t->n] = text; t->out_len[t->n] = (uint32_t)is;
    t->n++;
    return 1;
}
/* The blocks of the mapped file from *pos on, appended to t: at most max_rows of them, and only blocks that end at or before
 * `lim` -- the walk stands (*pos, and *text: the text bytes in front of it) at the first place where there is none.
 * 0 = no memory. */
static int bgzf_walk_map(const unsigned char *map, size_t size, size_t *pos, size_t lim, size_t max_rows, size_t *text, bgzf_rows_t *t) {
    for (size_t n = 0, bs, co, is; n < max_rows && *pos < lim; n++) {
        if (!bgzf_block(map + *pos, size - *pos, &bs, &co, &is) || is > 65536 || *pos + bs > lim) break;
        if (!bgzf_rows_add(t, *pos, bs, co, *text, is)) return 0;
        *text += is; *pos += bs;
    }
    return 1;
}
/* the whole file's table by one thread, through the mapping: 0 = t holds it (*text bytes of text), non-zero = bytes that
 * are no block somewhere before the file's end, or no memory */
int bgzf_walk_serial(const unsigned char *map, size_t size, bgzf_rows_t *t, size_t *text) {
    size_t pos = 0;
    t->n = 0; *text = 0;
    return !(bgzf_walk_map(map, size, &pos, size, (size_t)-1, text, t) && pos == size);
}

/* The BGZF header walk is a chain of dependent cache misses (122 000 blocks: 25 ms), so a team walks the file in
 * segments: every segment but the first finds a place where three valid block headers follow one another, walks from
 * there to the first block at or past its end, and the pieces are accepted only if every walk ends exactly where
 * the next one began -- then their concatenation IS the chain from offset 0.  Anything else: the serial walk.  The
 * team reads the file with pread (some 60 bytes per block), so that no page of the mapping is touched. */
typedef struct {
    int fd; size_t size, seg; int nseg;
    size_t *start, *end;                                 /* per segment: first block, where the walk stopped, */
    bgzf_rows_t *rows; int *bad;                         /* its blocks (without out_off) */
} bgzf_walk_t;
/* bgzf_block without the trailer: the first `have` bytes of a block that has `avail` bytes of file left */
static int bgzf_header(const unsigned char *p, size_t have, size_t avail, size_t *bsize, size_t *cdata_off) {
    if (have < 18 || p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) return 0;
    const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8), end = 12 + xlen;
    size_t off = 12, bs = 0;
    if (end > have) return 0;                            /* more extra fields than the walk reads: the serial walk takes the file */
    while (off + 4 <= end) {
        const size_t slen = (size_t)p[off + 2] | ((size_t)p[off + 3] << 8);
        if (p[off] == 'B' && p[off + 1] == 'C' && slen == 2 && off + 6 <= end) bs = ((size_t)p[off + 4] | ((size_t)p[off + 5] << 8)) + 1;
        off += 4 + slen;
    }
    if (bs < end + 8 || bs > avail) return 0;
    *bsize = bs; *cdata_off = end;
    return 1;
}
static void bgzf_walk_task(void *v, int k) {
    enum { WINDOW = 4 * 65536 + 256, HEAD = 60 };
    bgzf_walk_t *w = (bgzf_walk_t *)v;
    const size_t lim = k + 1 == w->nseg ? w->size : (size_t)(k + 1) * w->seg;
    size_t pos = (size_t)k * w->seg, bs, co, is;
    w->bad[k] = 1;
    if (k > 0) {                                         /* the first place in the segment where three valid blocks follow one another */
        unsigned char *win = (unsigned char *)malloc(WINDOW);
        if (!win) return;
        const size_t base = pos, wn = pread_full(w->fd, win, WINDOW, base), slim = lim - base < wn ? lim - base : wn;
        int found = 0;
        size_t o = 0;
        while (o < slim) {
            const unsigned char *c = (const unsigned char *)memchr(win + o, 31, slim - o);
            if (!c) break;
            o = (size_t)(c - win);
            size_t q = o;
            int chain = 0;
            while (chain < 3 && q < wn && bgzf_block(win + q, wn - q, &bs, &co, &is) && is <= 65536) { q += bs; chain++; }
            if (chain == 3 || (chain > 0 && base + q == w->size)) { found = 1; break; }
            o++;
        }
        free(win);
        if (!found) {
            if (slim < lim - base) return;               /* a segment longer than the window with no block start in the window: not BGZF as we know it */
            w->start[k] = w->end[k] = lim; w->bad[k] = 0; return;      /* no block begins in this segment */
        }
        pos = base + o;
    }
    w->start[k] = pos;
    bgzf_rows_t *t = &w->rows[k];
    int ok = bgzf_rows_reserve(t, w->seg / 8192 + 1024);
    unsigned char hb[4 + HEAD];
    size_t hn = ok && pos < lim ? pread_full(w->fd, hb + 4, HEAD, pos) : 0;      /* hb + 4: this block's first bytes */
    while (ok && pos < lim) {
        if (!bgzf_header(hb + 4, hn, w->size - pos, &bs, &co)) { ok = 0; break; }
        /* one read gets this block's last four bytes (ISIZE) and the next block's first ones */
        const size_t got = pread_full(w->fd, hb, 4 + HEAD, pos + bs - 4);
        if (got < 4) { ok = 0; break; }
        is = (size_t)hb[0] | ((size_t)hb[1] << 8) | ((size_t)hb[2] << 16) | ((size_t)hb[3] << 24);
        hn = got - 4;
        if (is > 65536 || !bgzf_rows_add(t, pos, bs, co, 0, is)) { ok = 0; break; }
        pos += bs;
    }
    w->end[k] = pos; w->bad[k] = !ok;
}
/* the whole file's table by the team: 0 = t holds it (*text bytes of text); non-zero = walk serially (t is empty) */
int bgzf_walk_parallel(int fd, size_t size, bgzf_rows_t *t, size_t *text) {
    enum { NSEG = 64 };
    if (size < (size_t)NSEG * 4096) return 1;
    bgzf_walk_t w;
    size_t start[NSEG], end[NSEG];
    bgzf_rows_t rows[NSEG]; int bad[NSEG];
    memset(rows, 0, sizeof rows);
    w.fd = fd; w.size = size; w.seg = size / NSEG; w.nseg = NSEG;
    w.start = start; w.end = end; w.rows = rows; w.bad = bad;
    io_pool_t tp;
    pool_init(&tp, default_io_threads());
    pool_run(&tp, bgzf_walk_task, &w, NSEG);
    pool_destroy(&tp);
    int ok = 1;
    size_t nb = 0, expect = 0;
    for (int k = 0; k < NSEG && ok; k++) {
        if (bad[k]) ok = 0;
        else if (rows[k].n == 0) { if (start[k] != end[k]) ok = 0; }       /* an empty segment: the chain passes over it */
        else { if (start[k] != expect) ok = 0; expect = end[k]; nb += rows[k].n; }
    }
    if (ok && expect != size) ok = 0;
    ok = ok && bgzf_rows_reserve(t, nb + 1);
    if (ok) {
        t->n = 0; *text = 0;
        for (int k = 0; k < NSEG; k++) {
            if (rows[k].n == 0) continue;
            memcpy(t->in_off + t->n, rows[k].in_off, rows[k].n * 8); memcpy(t->in_len + t->n, rows[k].in_len, rows[k].n * 4);
            memcpy(t->out_len + t->n, rows[k].out_len, rows[k].n * 4);
            t->n += rows[k].n;
        }
        for (size_t i = 0; i < nb; i++) { t->out_off[i] = *text; *text += t->out_len[i]; }
    }
    for (int k = 0; k < NSEG; k++) bgzf_rows_free(&rows[k]);
    return !ok;
}

/* ---- the stager: stretches of blocks decoded as their bytes arrive, their rows from one of two sources ------------------
 * The device scan (the default).  Walking the 490 000 block headers of a 4.6 GB file on the host takes 0.08 - 0.26 s of
 * dependent reads (beside the uploader's own reads of the same file) before the first block can be decoded.  So the stager
 * asks the device for the blocks in what has been uploaded so far (hpgv_bgzf_scan_dev finds the headers in the compressed
 * bytes and checks that they form a chain), decodes them, and goes on where the chain stands: the blocks of the first 8 MB
 * are decoded a few milliseconds after the file was opened, then stretches of 16 384 and 32 768 blocks as their bytes
 * arrive.  The text's size is not known in advance, so the text lies in a range of device addresses that is backed as the
 * table grows (dev_text_grow); the reader learns the text's end when the stager has seen the file's last block.  A stretch
 * of the file whose headers are not the ones bgzip writes is walked on the host (through the mapping).
 * The host's table (HPGV_BGZF_HOST_TABLE=1, HPGV_SERIAL_BGZF_WALK=1, or a text buffer that cannot grow: its size must be
 * known before it is allocated).  The table is complete (s->rows) before the stager starts; a stretch takes its next rows
 * when the uploader has passed them. */
enum { SCAN_ROWS_MAX = 131072, SCAN_SLOTS = 4 };
#define SCAN_RANGE_MAX ((size_t)2 << 30)
typedef struct {
    uint64_t *d_in_off, *d_out_off; uint32_t *d_in_len, *d_out_len; int32_t *d_status;       /* device rows of this stretch */
    bgzf_rows_t h;                                        /* and their host copy (for blocks the device refuses) */
    size_t text_end;
    void *stream;
} scan_slot_t;
typedef struct bgzf_stager {
    scan_slot_t slot[SCAN_SLOTS];
    int table;                                            /* the rows come from the host's table, not from the device scan */
    void *d_scratch; size_t scratch_bytes;                /* the device scan's */
    size_t chain_pos, text_pos, blocks;                   /* the chain stands at this file offset; text bytes and blocks before it */
    size_t first_n;                                       /* rows already in slot 0 (found when the path was chosen) */
    size_t rows_cap;                                      /* tests (HPGV_TEST_SCAN_ROWS): no stretch longer than this */
    size_t host_rows;                                     /* blocks the next walk on the host may take (doubles while the device finds no chain) */
} stager_t;

static int scan_slot_rows_to_host(scan_slot_t *q) {
    return hpgv_memcpy_d2h(CTX, q->h.in_off, q->d_in_off, q->h.n * 8, q->stream) == HPGV_OK
        && hpgv_memcpy_d2h(CTX, q->h.out_off, q->d_out_off, q->h.n * 8, q->stream) == HPGV_OK
        && hpgv_memcpy_d2h(CTX, q->h.in_len, q->d_in_len, q->h.n * 4, q->stream) == HPGV_OK
        && hpgv_memcpy_d2h(CTX, q->h.out_len, q->d_out_len, q->h.n * 4, q->stream) == HPGV_OK;
}
static int scan_slot_rows_to_device(scan_slot_t *q) {
    return hpgv_memcpy_h2d(CTX, q->d_in_off, q->h.in_off, q->h.n * 8, q->stream) == HPGV_OK
        && hpgv_memcpy_h2d(CTX, q->d_out_off, q->h.out_off, q->h.n * 8, q->stream) == HPGV_OK
        && hpgv_memcpy_h2d(CTX, q->d_in_len, q->h.in_len, q->h.n * 4, q->stream) == HPGV_OK
        && hpgv_memcpy_h2d(CTX, q->d_out_len, q->h.out_len, q->h.n * 4, q->stream) == HPGV_OK;
}
/* The next stretch's rows into slot q, on the host and on the device: up to max_rows blocks from where the chain stands.
 * 1 = q->h.n rows (0 rows: the file has ended) whose text ends at q->text_end, 0 = failure.  Two sources answer: */
/* ... the device scan, among the bytes that are up */
static int scan_next_rows(source_t *s, stager_t *S, scan_slot_t *q, size_t max_rows, int dbg, double T0) {
    const size_t avg = S->blocks ? S->chain_pos / S->blocks + 1 : 16384;
    size_t want = S->chain_pos + max_rows * avg;                      /* bytes that should hold that many blocks */
    /* the file's first stretch is whatever the first two segments hold (1 400 blocks of level 6): the header reader and
     * the pipeline wait for it, and a launch of 1 400 blocks takes as long as one of 4 096 (the time of one block) */
    if (S->blocks == 0 && want > ((size_t)8 << 20)) want = (size_t)8 << 20;
    for (;;) {
        if (S->chain_pos >= (size_t)s->size) return 1;
        const size_t have = wait_uploaded_some(s, want);
        if (!have) return 0;
        size_t hi = have;
        if (hi - S->chain_pos > SCAN_RANGE_MAX) hi = S->chain_pos + SCAN_RANGE_MAX;
        uint64_t res[4] = { 0, 0, 0, 0 };
        if (hpgv_bgzf_scan_dev(CTX, (const uint8_t *)s->d_comp, S->chain_pos, hi, S->text_pos, (int)max_rows, q->d_in_off, q->d_in_len,
                               q->d_out_off, q->d_out_len, S->d_scratch, S->scratch_bytes, res, q->stream) != HPGV_OK) return 0;
        if (res[0] > 0) {
            q->h.n = (size_t)res[0]; q->text_end = (size_t)res[2];
            if (!scan_slot_rows_to_host(q)) return 0;
            S->chain_pos = (size_t)res[1]; S->text_pos = q->text_end; S->blocks += q->h.n; S->host_rows = 64;
            if (dbg) fprintf(stderr, "stager: %zu blocks found up to byte %.1f MB (%.1f MB are up) at %.4f\n", q->h.n, S->chain_pos / 1e6, have / 1e6, now_s() - T0);
            return 1;
        }
        /* no block at the chain's position among the bytes that are up: it is not all there yet, or its header is not bgzip's */
        if (hi < (size_t)s->size && hi - S->chain_pos < ((size_t)1 << 17)) { want = hi + ((size_t)1 << 20); continue; }
        size_t end = S->chain_pos, tend = S->text_pos;
        if (S->host_rows < 64) S->host_rows = 64;
        if (!bgzf_walk_map(s->map, (size_t)s->size, &end, hi, S->host_rows < max_rows ? S->host_rows : max_rows, &tend, &q->h)) return 0;
        S->host_rows *= 2;                                            /* a few blocks, then the device again; more if it still finds none */
        if (q->h.n == 0) {
            if (hi < (size_t)s->size) { want = hi + ((size_t)1 << 20); continue; }      /* a block that ends beyond what is up */
            return 0;                                                 /* bytes that are no block */
        }
        if (dbg) fprintf(stderr, "stager: %zu blocks walked on the host from byte %zu at %.4f\n", q->h.n, S->chain_pos, now_s() - T0);
        q->text_end = tend;
        if (!scan_slot_rows_to_device(q)) return 0;
        S->chain_pos = end; S->text_pos = tend; S->blocks += q->h.n;
        return 1;
    }
}
/* ... and the host's table, once the uploader has passed the stretch's last block */
static int table_next_rows(source_t *s, stager_t *S, scan_slot_t *q, size_t max_rows, int dbg, double T0) {
    const bgzf_rows_t *t = &s->rows;
    const size_t a = S->blocks, n = t->n - a < max_rows ? t->n - a : max_rows;
    if (n == 0) return 1;
    const size_t hi = (size_t)t->in_off[a + n - 1] + t->in_len[a + n - 1] + 8;      /* + the last block's trailer: its CRC-32 is checked */
    if (wait_uploaded_some(s, hi) < hi) return 0;
    if (dbg) fprintf(stderr, "stager: [%zu,%zu) is up, to byte %.1f MB, at %.4f\n", a, a + n, hi / 1e6, now_s() - T0);
    memcpy(q->h.in_off, t->in_off + a, n * 8); memcpy(q->h.out_off, t->out_off + a, n * 8);
    memcpy(q->h.in_len, t->in_len + a, n * 4); memcpy(q->h.out_len, t->out_len + a, n * 4);
    q->h.n = n; q->text_end = (size_t)t->out_off[a + n - 1] + t->out_len[a + n - 1];
    if (!scan_slot_rows_to_device(q)) return 0;
    S->chain_pos = hi; S->text_pos = q->text_end; S->blocks += n;
    return 1;
}
static int next_rows(source_t *s, stager_t *S, scan_slot_t *q, size_t max_rows, int dbg, double T0) {
    q->h.n = 0; q->text_end = S->text_pos;
    return S->table ? table_next_rows(s, S, q, max_rows, dbg, T0) : scan_next_rows(s, S, q, max_rows, dbg, T0);
}
/* How many blocks the next stretch may hold when `launched` blocks have been launched: a short first stretch, which the
 * header reader and the pipeline wait for (a wave per block: 1.5 ms), then longer ones.  Behind the device scan 16 384 and
 * 32 768 blocks at a time: a stretch is launched when its bytes are up, and the decoder (23 GB/s of bgzip's level-6 bytes)
 * is not much slower than the bus -- behind stretches that double, the device waited for the next one's bytes.  With the
 * host's table the uploader is well ahead when the table is there: stretches that double from 32 768 up to 131 072 blocks,
 * and a small file in one launch. */
static size_t stretch_rows(const source_t *s, const stager_t *S, size_t launched) {
    enum { FIRST = 4096 };
    size_t rows = launched == 0 ? FIRST : launched < FIRST + 16384 ? 16384 : 32768;
    if (S->table)
        rows = launched == 0 ? (s->rows.n <= 3 * FIRST ? s->rows.n : FIRST)
             : launched < FIRST + 32768 ? 32768 : launched < FIRST + 3 * 32768 ? 65536 : 131072;
    return S->rows_cap && rows > S->rows_cap ? S->rows_cap : rows;
}
/* Block i of slot q, the file's block b, when the device decoder is through with it: one it did not take (or, in tests,
 * every HPGV_TEST_GPU_INFLATE_REFUSE_EVERY-th block) is decoded by the host and its text patched in.  0 = the block is bad.
 * That hook patches the text the device counted; HPGV_TEST_GPU_INFLATE_DAMAGE_EVERY=n stands for a decoder that wrote WRONG
 * bytes: behind the decoder's launch and in front of the CRC check's (damage_decoded, on the slot's stream) 32 bytes in the
 * middle of every block b with b % n == 0 and 64 bytes of text or more are overwritten with newlines and TABs.  The CRC check
 * then refuses the block, the host patches it here, and the tile records the check counted from the damaged text must not be
 * used (hpgv.h "hpgv_bgzf_verify_tiles_dev").  Both hooks number the blocks alike: from 0 in the file, or in the part. */
#define NT4 '\n', '\t', '\n', '\t', '\n', '\t', '\n', '\t'
static const char DAMAGE_PATTERN[32] = { NT4, NT4, NT4, NT4 };
#undef NT4
static int damage_decoded(source_t *s, const scan_slot_t *q, size_t first_block) {
    const size_t every = (size_t)g_env.test_damage_every;
    for (size_t i = 0; every && i < q->h.n; i++) {
        if ((first_block + i) % every != 0 || q->h.out_len[i] < 64) continue;
        /* (only queued; the pattern is static and never written, so it is "left alone" for as long as anyone may read it) */
        if (hpgv_memcpy_h2d_async(CTX, (char *)s->d_text + q->h.out_off[i] + q->h.out_len[i] / 2 - sizeof DAMAGE_PATTERN / 2, DAMAGE_PATTERN,
                                  sizeof DAMAGE_PATTERN, q->stream) != HPGV_OK) return 0;
    }
    return 1;
}
static int patch_if_refused(source_t *s, const scan_slot_t *q, size_t i, size_t b, int32_t status, unsigned char *tmp) {
    const size_t every = (size_t)g_env.test_refuse_every;
    if (!status && !(every && b % every == 0)) return 1;
    return !inflate_block(s->map + q->h.in_off[i], q->h.in_len[i], tmp, q->h.out_len[i])
        && hpgv_memcpy_h2d(CTX, (char *)s->d_text + q->h.out_off[i], tmp, q->h.out_len[i], q->stream) == HPGV_OK;
}

/* the stretches go through a ring of SCAN_SLOTS slots: the stager finds and launches them as their bytes arrive, the
 * publisher waits for them in file order, patches what the device refused and hands the text to the reader -- neither
 * waits for the other's event */
typedef struct {
    source_t *s; stager_t *S;
    pthread_mutex_t mu; pthread_cond_t cv;
    size_t n_launched, n_published;                       /* stretches; slot k % SCAN_SLOTS holds stretch k */
    int launch_done, bad;
    double T0; int dbg;
} scan_ring_t;
static void *bgzf_publisher(void *v) {
    scan_ring_t *R = (scan_ring_t *)v;
    source_t *s = R->s;
    (void)SRC_CTX(s);                                               /* this thread works on the part's member device from here on */
    unsigned char *tmp = (unsigned char *)malloc(65536);
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * SCAN_ROWS_MAX);
    int ok = tmp && st;
    size_t done_blocks = 0;
    for (size_t k = 0; ok; k++) {
        pthread_mutex_lock(&R->mu);
        while (R->n_launched <= k && !R->launch_done && !R->bad) pthread_cond_wait(&R->cv, &R->mu);
        const int have = R->n_launched > k && !R->bad;
        pthread_mutex_unlock(&R->mu);
        if (!have) break;
        scan_slot_t *q = &R->S->slot[k % SCAN_SLOTS];
        ok = hpgv_memcpy_d2h(CTX, st, q->d_status, q->h.n * 4, q->stream) == HPGV_OK;         /* synchronises that stream */
        for (size_t i = 0; ok && i < q->h.n; i++) ok = patch_if_refused(s, q, i, done_blocks + i, st[i], tmp);
        done_blocks += q->h.n;
        if (R->dbg) fprintf(stderr, "stager: decoded up to block %zu at %.4f\n", done_blocks, now_s() - R->T0);
        if (ok) {
            pthread_mutex_lock(&s->g_mu);
            s->g_done = done_blocks;
            s->dev_ready = q->text_end;
            pthread_cond_broadcast(&s->g_cv);
            pthread_mutex_unlock(&s->g_mu);
        }
        pthread_mutex_lock(&R->mu);
        R->n_published = k + 1;
        if (!ok) R->bad = 1;
        pthread_cond_broadcast(&R->cv);
        pthread_mutex_unlock(&R->mu);
    }
    if (!ok) { pthread_mutex_lock(&R->mu); R->bad = 1; pthread_cond_broadcast(&R->cv); pthread_mutex_unlock(&R->mu); }
    free(tmp); free(st);
    return NULL;
}
/* the stager's own state: the slots' streams (slot 0's is s->cstream, which stays), their rows on the host and the device */
static void stager_free(source_t *s) {
    stager_t *S = s->stager;
    if (!S) return;
    for (int q = 1; q < SCAN_SLOTS; q++) stream_put(s->c_low, S->slot[q].stream);
    for (int q = 0; q < SCAN_SLOTS; q++) bgzf_rows_free(&S->slot[q].h);
    free(S); s->stager = NULL;
    if (s->d_scan) { (void)hpgv_dev_free(CTX, s->d_scan); s->d_scan = NULL; }
}
static void *bgzf_stager(void *v) {
    source_t *s = (source_t *)v;
    (void)SRC_CTX(s);                                               /* this thread works on the part's member device from here on */
    stager_t *S = s->stager;
    scan_ring_t R;
    memset(&R, 0, sizeof R);
    R.s = s; R.S = S; R.dbg = (g_env.run_trace != 0); R.T0 = now_s();
    const int dbg = R.dbg; const double T0 = R.T0;
    pthread_mutex_init(&R.mu, NULL); pthread_cond_init(&R.cv, NULL);
    pthread_t pub;
    int ok = pthread_create(&pub, NULL, bgzf_publisher, &R) == 0;
    const int have_pub = ok;
    size_t launched = 0;
    for (size_t k = 0; ok; k++) {
        pthread_mutex_lock(&R.mu);                                   /* a free slot */
        while (k >= R.n_published + SCAN_SLOTS && !R.bad) pthread_cond_wait(&R.cv, &R.mu);
        ok = !R.bad;
        pthread_mutex_unlock(&R.mu);
        if (!ok) break;
        scan_slot_t *q = &S->slot[k % SCAN_SLOTS];
        if (k > 0 || !S->first_n) ok = next_rows(s, S, q, stretch_rows(s, S, launched), dbg, T0);      /* (else: found when the path was chosen) */
        if (!ok || q->h.n == 0) break;                               /* (no rows: the file has ended) */
        if (k == 1) {                                                /* launches side by side finish together: the first stretch, which the */
            pthread_mutex_lock(&R.mu);                               /* header reader waits for, decodes alone (1.5 ms instead of 6) */
            while (R.n_published < 1 && !R.bad) pthread_cond_wait(&R.cv, &R.mu);
            ok = !R.bad;
            pthread_mutex_unlock(&R.mu);
            if (!ok) break;
        }
        if (!S->table)                                               /* (the table's text was allocated whole) */
            ok = dev_text_grow(s->d_text, q->text_end + 16 + (q->text_end >> 4), &s->d_text_cap)      /* some room ahead: growing waits for the kernels that run */
              || dev_text_grow(s->d_text, q->text_end + 16, &s->d_text_cap);
        ok = ok && hpgv_inflate_blocks_dev(CTX, (const uint8_t *)s->d_comp, q->d_in_off, q->d_in_len, q->d_out_off, q->d_out_len,
                                           (int)q->h.n, (uint8_t *)s->d_text, q->d_status, q->stream) == HPGV_OK;
        ok = ok && damage_decoded(s, q, launched);                   /* (tests: a decoder that wrote wrong bytes) */
        if (g_env.bgzf_verify)                                       /* the blocks' CRC-32, on the device behind the decoder */
            ok = ok && hpgv_bgzf_verify_tiles_dev(CTX, (const uint8_t *)s->d_comp, q->d_in_off, q->d_in_len, q->d_out_off, q->d_out_len,
                                                  (int)q->h.n, (const uint8_t *)s->d_text, q->d_status, s->d_tiles, (uint64_t)s->n_tiles, q->stream) == HPGV_OK;
        if (!ok) break;
        if (dbg && k == 0) fprintf(stderr, "stager: first stretch launched at %.4f\n", now_s() - T0);
        launched += q->h.n;
        pthread_mutex_lock(&R.mu);
        R.n_launched = k + 1;
        pthread_cond_broadcast(&R.cv);
        pthread_mutex_unlock(&R.mu);
        if (S->chain_pos >= (size_t)s->size) break;
    }
    pthread_mutex_lock(&R.mu);
    R.launch_done = 1;
    if (!ok) R.bad = 1;
    pthread_cond_broadcast(&R.cv);
    pthread_mutex_unlock(&R.mu);
    if (have_pub) pthread_join(pub, NULL);
    ok = ok && !R.bad;
    pthread_mutex_destroy(&R.mu); pthread_cond_destroy(&R.cv);
    for (int q = 0; q < SCAN_SLOTS; q++) if (S->slot[q].stream) (void)hpgv_stream_sync(CTX, S->slot[q].stream);      /* after a failure launches may still be running */
    pthread_mutex_lock(&s->g_mu);
    if (!ok) s->g_err = 1;
    else { s->dev_len = S->text_pos; s->dev_len_known = 1; s->g_nb = S->blocks; }
    s->g_finished = 1;
    pthread_cond_broadcast(&s->g_cv);
    pthread_mutex_unlock(&s->g_mu);
    upload_cancel(s);                                               /* the compressed bytes are freed below: the uploader must be through */
    if (dbg) fprintf(stderr, "stager: finished (%zu blocks, %.1f MB of text) at %.4f\n", S->blocks, S->text_pos / 1e6, now_s() - T0);
    stager_free(s);                                                 /* only the text is needed from here on */
    bgzf_rows_free(&s->rows);
    if (s->d_comp) { (void)hpgv_dev_free(CTX, s->d_comp); s->d_comp = NULL; }
    return NULL;
}

/* the stager's state and what it works with: the reader's stream and the decoder's (at the lowest priority if `low`: the
 * batches' kernels go first whenever a compute unit has room), the slots' rows, and for the device scan its scratch.
 * 0 = failed; what there is, is bgzf_stage_release's */
static int stager_new(source_t *s, int low, int table) {
    stager_t *S = (stager_t *)calloc(1, sizeof *S);
    if (!S) return 0;
    s->stager = S; s->c_low = low;
    S->table = table;
    S->rows_cap = g_env.test_scan_rows > 0 ? (size_t)g_env.test_scan_rows : 0;
    int ok = stream_get(0, &s->rstream) == HPGV_OK && stream_get(low, &s->cstream) == HPGV_OK;
    const size_t slot_bytes = (size_t)SCAN_ROWS_MAX * 28;
    S->scratch_bytes = table ? 0 : hpgv_bgzf_scan_scratch_bytes(SCAN_RANGE_MAX + 16, SCAN_ROWS_MAX);
    if (ok) ok = hpgv_dev_alloc(CTX, slot_bytes * SCAN_SLOTS + S->scratch_bytes + 256, &s->d_scan) == HPGV_OK;
    for (int k = 0; ok && k < SCAN_SLOTS; k++) {
        scan_slot_t *q = &S->slot[k];
        char *d = (char *)s->d_scan + (size_t)k * slot_bytes;
        q->d_in_off = (uint64_t *)d; q->d_out_off = (uint64_t *)(d + (size_t)SCAN_ROWS_MAX * 8);
        q->d_in_len = (uint32_t *)(d + (size_t)SCAN_ROWS_MAX * 16); q->d_out_len = (uint32_t *)(d + (size_t)SCAN_ROWS_MAX * 20);
        q->d_status = (int32_t *)(d + (size_t)SCAN_ROWS_MAX * 24);
        ok = bgzf_rows_reserve(&q->h, SCAN_ROWS_MAX);
        if (k == 0) q->stream = s->cstream; else ok = ok && stream_get(low, &q->stream) == HPGV_OK;
    }
    if (ok && !table) S->d_scratch = (char *)s->d_scan + slot_bytes * SCAN_SLOTS;
    return ok;
}
/* hands the file to the stager thread; 0 = no thread */
static int stager_start(source_t *s) {
    s->dev_pos = 0; s->dev_ready = 0; s->g_done = 0; s->g_err = 0; s->g_finished = 0;
    if (pthread_create(&s->g_thread, NULL, bgzf_stager, s) != 0) return 0;
    s->g_started = 1;
    s->map_pos = (size_t)s->size;                                    /* the CPU path has nothing left to do */
    return 1;
}
/* Everything a stage attempt holds, whether it was taken or not (the stager thread, if there was one, has ended): the
 * stager's state, the table, the text and its tiles, the streams.  The compressed bytes and the sync objects go with them
 * unless the uploader is still running (upload_cancel first): a file the device scan does not take goes on to the host's
 * table with its upload under way. */
void bgzf_stage_release(source_t *s) {
    bgzf_rows_free(&s->rows);
    if (g_ctx) {
        stager_free(s);
        if (s->d_text) { dev_text_put(s->d_text, s->d_text_cap, s->d_text_kind); s->d_text = NULL; }
        tiles_free(s);
        stream_put(0, s->rstream); s->rstream = NULL;
        stream_put(s->c_low, s->cstream); s->cstream = NULL; s->c_low = 0;
        if (s->d_comp && !s->u_started) { (void)hpgv_dev_free(CTX, s->d_comp); s->d_comp = NULL; }
    }
    if (s->g_sync && !s->u_started) { pthread_mutex_destroy(&s->g_mu); pthread_cond_destroy(&s->g_cv); s->g_sync = 0; }
}

/* the device scan as the source: 0 = the stager has the file; 1 = not taken (the caller goes on with the host's table) */
static int bgzf_stream_stage(source_t *s) {
    const int dbg = (g_env.run_trace != 0); const double T0 = now_s();
    int ok = stager_new(s, !g_env.no_low_priority, 0);
    stager_t *S = s->stager;
    if (!S) return 1;
    if (dbg) fprintf(stderr, "stage: streams and tables at %.4f\n", now_s() - T0);
    /* the first blocks, from the file's first megabytes: is this a file the device can chain, and how much text is it? */
    ok = ok && next_rows(s, S, &S->slot[0], stretch_rows(s, S, 0), dbg, T0) && S->slot[0].h.n > 0;
    size_t est = 0;
    if (ok) {
        /* committed at once, with room (growing later waits for the kernels that are running) */
        est = (size_t)((double)S->text_pos / (double)S->chain_pos * (double)s->size * 1.10) + ((size_t)128 << 20);
        if (S->chain_pos >= (size_t)s->size) est = S->text_pos + 16;
        if (est > ((size_t)48 << 30)) ok = 0;                        /* as with the host's table: such a text stays on the host path, */
        if (S->chain_pos >= (size_t)s->size && S->blocks < 256 && !s->is_part && !s->mp) ok = 0;      /* and a small file is as quick there */
    }
    const long tp = g_env.test_text_estimate_percent;              /* tests: a text that outgrows what was committed for it */
    if (ok && tp > 0 && S->chain_pos < (size_t)s->size) {
        est = (size_t)((double)S->text_pos / (double)S->chain_pos * (double)s->size) / 100 * (size_t)tp;
        if (est < S->text_pos + 16) est = S->text_pos + 16;
        dev_text_drop_cached();
    }
    if (ok) {
        s->text_est = S->chain_pos >= (size_t)s->size ? S->text_pos : (size_t)((double)S->text_pos / (double)S->chain_pos * (double)s->size);
        s->d_text = dev_text_get(est, &s->d_text_cap, &s->d_text_kind);
        ok = s->d_text != NULL && ((s->d_text_kind == DEV_TEXT_GROWS && !g_env.no_growing_text) || S->chain_pos >= (size_t)s->size);
        if (ok) tiles_alloc(s, est);
    }
    if (dbg) fprintf(stderr, "stage: first %zu blocks found, text estimate %.1f MB, %s at %.4f\n", S->slot[0].h.n, est / 1e6, ok ? "streaming" : "not taken", now_s() - T0);
    if (ok) {
        S->first_n = S->slot[0].h.n;
        s->dev_len = 0; s->dev_len_known = 0; s->g_nb = 0;
        ok = stager_start(s);
    }
    if (!ok) bgzf_stage_release(s);
    return !ok;
}
/* the host's table as the source: walked by the team or by one thread, complete before the text is allocated (at its
 * size) and the stager starts.  0 = the stager has the file; 1 = not taken */
static int bgzf_table_stage(source_t *s) {
    const int dbg = (g_env.run_trace != 0); const double T0 = now_s();
    size_t text = 0;
    int ok = 1;
    if (g_env.serial_bgzf_walk || bgzf_walk_parallel(s->fd, (size_t)s->size, &s->rows, &text)) {
        if (dbg) fprintf(stderr, "stage: serial walk\n");
        ok = bgzf_walk_serial(s->map, (size_t)s->size, &s->rows, &text) == 0;
    }
    if (dbg) fprintf(stderr, "stage: walk %.4f\n", now_s() - T0);
    const size_t nb = s->rows.n;
    if (ok && (nb < 256 || nb > 0x7FFFFFFFu || text > ((size_t)48 << 30))) ok = 0;     /* a small file is as quick on the host */
    ok = ok && stager_new(s, 0, 1);
    if (ok) { s->text_est = text; s->d_text = dev_text_get(text + 16, &s->d_text_cap, &s->d_text_kind); ok = s->d_text != NULL; }
    if (ok) tiles_alloc(s, text + 16);
    if (dbg) fprintf(stderr, "stage: alloc %.4f\n", now_s() - T0);
    if (ok) {
        s->dev_len = text; s->dev_len_known = 1; s->g_nb = nb;
        ok = stager_start(s);
    }
    return !ok;
}

/* ---- a bgzip file on SEVERAL devices (a group context: HPGV_DEVICES, hpgv_host_init_devices; --num-threads / the devices
 * option of shared_options.c:60-61 has no such notion: the reference reads the file with one thread).  BGZF blocks are
 * independent, so the file is cut at block starts into one contiguous PART per member: every part goes up ITS device's own
 * link (the upload is what a run of the device path waits for), is decoded and kept there, and its windows are tokenized and
 * scanned there.  Each part is staged by the streaming stager exactly as a whole file is (a source_t whose map / size /
 * file_off describe the part).  The reader walks the parts in file order; a part's text ends inside a line as a rule: the
 * line's head (the end of part k) and tail (the start of part k + 1) come back to the host, and the joined line goes through
 * the ordinary host-text entry as a batch of one line between the two parts' windows (read_lines_dev). ---- */
/* one part (or, when the parts are given up, nothing): 0 = the streaming stager has it */
static int part_stream_stage(source_t *s) {
    const ctx_saved_t saved = SRC_CTX(s);
    s->gpu_tried = 1;
    const int taken = upload_start(s) && bgzf_stream_stage(s) == 0;
    if (!taken) { upload_cancel(s); bgzf_stage_release(s); }          /* nothing is left behind */
    ctx_back(saved);
    return !taken;
}
/* the first block start at or after `from` from which four blocks chain (a header's magic inside compressed data does not) */
static size_t bgzf_find_block_start(const source_t *s, size_t from) {
    const size_t size = (size_t)s->size, lim = from + ((size_t)1 << 20) < size ? from + ((size_t)1 << 20) : size;
    for (size_t pos = from; pos + 28 <= lim; pos++) {
        if (s->map[pos] != 31 || s->map[pos + 1] != 139) continue;
        size_t q = pos;
        int n = 0;
        while (n < 4 && q < size) {
            size_t bs, co, is;
            if (!bgzf_block(s->map + q, size - q, &bs, &co, &is) || is > 65536) break;
            q += bs; n++;
        }
        if (n == 4 || (n > 0 && q == size)) return pos;
    }
    return 0;
}
/* 0 = the file is staged in parts (s is part 0); 1 = not taken, s is as it was */
static int bgzf_parts_stage(source_t *s) {
    const int G = g_ctx ? hpgv_group_size(g_ctx) : 1;
    if (G < 2 || g_env.bgzf_one_device || g_env.no_device_windows || g_env.bgzf_host_table || g_env.serial_bgzf_walk || g_env.no_growing_text) return 1;
    const size_t part_min = g_env.bgzf_part_min_kb > 0 ? (size_t)g_env.bgzf_part_min_kb << 10 : (size_t)64 << 20;      /* (tests: parts of small files) */
    int n = G < MEMBERS_MAX ? G : MEMBERS_MAX;
    if ((size_t)s->size / part_min < (size_t)n) n = (int)((size_t)s->size / part_min);
    if (n < 2) return 1;
    size_t b[MEMBERS_MAX + 1];
    b[0] = 0; b[n] = (size_t)s->size;
    for (int k = 1; k < n; k++) {
        b[k] = bgzf_find_block_start(s, (size_t)s->size / (size_t)n * (size_t)k);
        if (b[k] == 0 || b[k] <= b[k - 1]) return 1;
    }
    src_parts_t *mp = (src_parts_t *)calloc(1, sizeof *mp);
    if (!mp) return 1;
    mp->n = n; mp->p[0] = s; mp->whole_size = s->size;
    const int dbg = (g_env.run_trace != 0);
    int ok = 1;
    for (int k = 1; ok && k < n; k++) {                              /* the later parts first: if one of them is not taken, part 0 is still the whole file */
        source_t *p = (source_t *)calloc(1, sizeof *p);
        if (!p) { ok = 0; break; }
        p->kind = SRC_BGZF; p->fd = dup(s->fd); p->is_part = 1;
        p->map_base = s->map_base; p->map_len = s->map_len;
        p->map = s->map + b[k]; p->size = (off_t)(b[k + 1] - b[k]); p->file_off = (off_t)b[k];
        p->ctx = hpgv_group_member(g_ctx, k); p->member = k;
        mp->p[k] = p;
        ok = p->fd >= 0 && p->ctx && part_stream_stage(p) == 0;
        if (ok) p->map_pos = (size_t)p->size;
    }
    if (ok) {
        s->ctx = hpgv_group_member(g_ctx, 0); s->member = 0; s->mp = mp; s->size = (off_t)b[1];
        ok = part_stream_stage(s) == 0;
        if (!ok) { s->ctx = NULL; s->mp = NULL; s->size = mp->whole_size; s->gpu_tried = 0; }
    }
    if (!ok) {
        for (int k = 1; k < n; k++) if (mp->p[k]) { source_close(mp->p[k]); free(mp->p[k]); }
        free(mp);
        if (dbg) fprintf(stderr, "stage: the file is not taken in parts\n");
        return 1;
    }
    if (dbg) { fprintf(stderr, "stage: %d parts, one per device, cut at bytes", n); for (int k = 1; k < n; k++) fprintf(stderr, " %zu", b[k]); fprintf(stderr, "\n"); }
    s->map_pos = (size_t)s->size;                                    /* the CPU path has nothing left to do */
    return 0;
}

int bgzf_gpu_stage(source_t *s) {
    s->gpu_tried = 1;
    if (g_env.no_gpu_inflate || !g_ctx || s->map_pos != 0) return 1;
    if ((size_t)s->size < ((size_t)64 << 10)) return 1;             /* a tiny file is as quick on the host (the block count decides below) */
    if (!s->is_part && !s->mp && bgzf_parts_stage(s) == 0) return 0;
    if (!upload_start(s)) return 1;
    if (!g_env.bgzf_host_table && !g_env.serial_bgzf_walk && bgzf_stream_stage(s) == 0) return 0;
    if (bgzf_table_stage(s) == 0) return 0;
    upload_cancel(s);                                               /* not a file for the device path after all */
    bgzf_stage_release(s);
    return 1;
}
