// hpgv_lines_capi.hip -- C ABI of the line tools (include/hpgv.h): stable partition and multi-way split of a text's lines on
// the device (hpg-var-vcf filter / split), on the caller's buffers (*_dev) or on the text hpgv_filter_text tokenized and
// holds.  The tokenizer and text_front are in hpgv_text_capi.hip; this unit includes hpgv_text_kernels.h for the heads'
// three-launch scan (k_head_bases), which the partition's offsets reuse.
#include "hpgv_internal.h"
#include <climits>
#include "hpgv_text_kernels.h"
#include "hpgv_partition_kernels.h"

extern "C" {

/* ---- stable partition of lines: kept lines, then the others (hpg-var-vcf filter: .filtered / .rejected) ---- */

size_t hpgv_lines_partition_scratch_bytes(int n_lines) {
    if (n_lines <= 0) return 0;
    const size_t hb = ((size_t)n_lines + 1023) / 1024;
    return ((size_t)n_lines + 1 + hb) * sizeof(unsigned long long);
}

// the launches of one partition on `st`: kept_off and the block sums in d_scratch, then the copy
static int partition_launch(hpgv_ctx *ctx, const char *d_text, const unsigned long long *d_line_off, int n_lines,
                            const uint8_t *d_keep, char *d_out, unsigned long long *d_kept_bytes, void *d_scratch, hipStream_t st) {
    if (n_lines == 0) {
        if (d_kept_bytes) HIPCHK(ctx, hipMemsetAsync(d_kept_bytes, 0, sizeof(unsigned long long), st));
        return HPGV_OK;
    }
    const int hb = (n_lines + 1023) / 1024;
    unsigned long long *kept_off = (unsigned long long *)d_scratch, *block = kept_off + (size_t)n_lines + 1;
    hipLaunchKernelGGL(hpgv::k_kept_sums, dim3((unsigned)hb), dim3(1024), 0, st, d_line_off, d_keep, n_lines, block);
    hipLaunchKernelGGL(hpgv::k_head_bases, dim3(1), dim3(1024), 0, st, block, hb);
    hipLaunchKernelGGL(hpgv::k_kept_offsets, dim3((unsigned)hb), dim3(1024), 0, st, d_line_off, d_keep, n_lines,
                       (const unsigned long long *)block, kept_off);
    // whole waves striding over the lines: at least one line per wave, at most 8 workgroups of 4 waves per CU
    const long cap = 8L * (ctx->n_cus > 0 ? ctx->n_cus : 256);
    const long blocks = std::min<long>(((long)n_lines + 3) / 4, cap);
#ifdef HPGV_ABLATION
    if (ctx->part_aligned)
        hipLaunchKernelGGL(hpgv::k_part_copy<1>, dim3((unsigned)blocks), dim3(256), 0, st, d_text, d_line_off, n_lines, d_keep,
                           (const unsigned long long *)kept_off, d_out, d_kept_bytes);
    else
#endif
        hipLaunchKernelGGL(hpgv::k_part_copy<0>, dim3((unsigned)blocks), dim3(256), 0, st, d_text, d_line_off, n_lines, d_keep,
                           (const unsigned long long *)kept_off, d_out, d_kept_bytes);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_lines_partition_dev(hpgv_ctx *ctx, const char *d_text, const uint64_t *d_line_off, int n_lines, const uint8_t *d_keep,
                             char *d_out, uint64_t *d_kept_bytes, void *d_scratch, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_lines < 0 || (n_lines > 0 && (!d_text || !d_line_off || !d_keep || !d_out || !d_scratch)))
        return fail(ctx, HPGV_ERR_INVALID, "bad lines_partition_dev arguments");
    DeviceGuard g(ctx->device);
    return partition_launch(ctx, d_text, (const unsigned long long *)d_line_off, n_lines, d_keep, d_out,
                            (unsigned long long *)d_kept_bytes, d_scratch, (hipStream_t)stream);
    HPGV_ABI_CATCH(ctx)
}

// the hold hpgv_filter_text left on `host_text` (taken out of the list), or false
static bool take_held(hpgv_ctx *ctx, const char *host_text, hpgv_ctx::TextHeld *out) {
    std::lock_guard<std::mutex> lk(ctx->alias_mu);
    for (size_t i = 0; i < ctx->text_held.size(); ++i)
        if (ctx->text_held[i].host_text == host_text) { *out = ctx->text_held[i]; ctx->text_held.erase(ctx->text_held.begin() + (long)i); return true; }
    return false;
}

int hpgv_filter_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                     uint64_t *line_off, uint32_t *field_off, int32_t *status) {
    HPGV_ABI_TRY
    if (is_group(ctx)) for (hpgv_ctx *m : ctx->members) (void)hpgv_text_partition(m, text, nullptr, 0, nullptr, 0, nullptr, nullptr);   // an earlier hold on this text
    GROUP_DEAL_TEXT(ctx, text, hpgv_filter_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (!n_lines || max_lines < 0 || !text || (max_lines > 0 && (!line_off || !field_off || !status)))
        return fail(ctx, HPGV_ERR_INVALID, "bad filter_text arguments");
    (void)hpgv_text_partition(ctx, text, nullptr, 0, nullptr, 0, nullptr, nullptr);
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S, false))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    if (*n_lines > max_lines) return HPGV_OK;                      // the caller grows its arrays and calls again
    const char *d_src = text_on_device(ctx, text);
    hpgv_ctx::TextHeld h{text, s, d_src ? d_src : s->text.as<const char>(), TextMeta(s->meta, max_lines).line_off(), S.n};
    {
        std::lock_guard<std::mutex> lk(ctx->alias_mu);
        ctx->text_held.push_back(h);
    }
    lease.s = nullptr;                                              // the slot stays leased to the hold
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

// what the _bgzf twins ask for beyond the plain call: the parts deflated into BGZF members on the device before they are
// copied back (hpgv_bgzf_deflate_dev with the primitive's own device-side offsets as segment bounds)
struct BgzfWant {
    int want_rest = 1;                  // partition: 0 = the other lines are neither deflated nor copied
    uint64_t *comp = nullptr;           // partition: the two parts' member bytes
    uint8_t *last = nullptr;            // the last text byte of every part ('\n' for an empty one)
};

// the parts' last bytes, for a writer that must end a file's last line
static __global__ void k_seg_last_bytes(const char *__restrict__ text, const unsigned long long *__restrict__ seg_off, int n_segs, uint8_t *__restrict__ last) {
    for (int s = (int)threadIdx.x; s < n_segs; s += (int)blockDim.x) last[s] = seg_off[s + 1] > seg_off[s] ? (uint8_t)text[seg_off[s + 1] - 1] : (uint8_t)'\n';
}
// the two segments of a partition: [0, kept) and [kept, total) -- the second empty when the caller does not want it
static __global__ void k_part_segs(const unsigned long long *__restrict__ kept, unsigned long long total, int want_rest, unsigned long long *__restrict__ seg_off) {
    if (threadIdx.x == 0) { seg_off[0] = 0; seg_off[1] = *kept; seg_off[2] = want_rest ? total : *kept; }
}

// the text in the slot's `parts`, n_segs segments bounded by d_seg_off, as members in its `members`; d_res: seg_out_off[n_segs + 1],
// then a last byte per segment.  Queued on the slot's stream.
static int deflate_parts(hpgv_ctx *ctx, Slot *s, size_t total, const unsigned long long *d_seg_off, int n_segs, unsigned long long *d_res) {
    HIPCHK(ctx, s->members.reserve_slack(hpgv_bgzf_deflate_bound(total, n_segs) + 16));
    HIPCHK(ctx, s->dfl.reserve_slack(hpgv_bgzf_deflate_scratch_bytes(total, n_segs) + 16));
    if (const int rc = hpgv_bgzf_deflate_launch(ctx, s->parts.as<const char>(), d_seg_off, n_segs, s->members.as<uint8_t>(), d_res, s->dfl.p, s->stream)) return rc;
    hipLaunchKernelGGL(k_seg_last_bytes, dim3(1), dim3(256), 0, s->stream, s->parts.as<const char>(), d_seg_off, n_segs, (uint8_t *)(d_res + n_segs + 1));
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

static int text_partition(hpgv_ctx *ctx, const char *text, const uint8_t *keep, int n_lines, char *out, size_t out_cap,
                          uint64_t *kept_bytes, uint64_t *total_bytes, const BgzfWant *Z) {
    {
    if (is_group(ctx)) {
        int rc = HPGV_OK, found = 0;
        for (hpgv_ctx *m : ctx->members) {
            bool held;
            { std::lock_guard<std::mutex> lk(m->alias_mu); held = false; for (const auto &h : m->text_held) if (h.host_text == text) held = true; }
            if (held) { found = 1; rc = text_partition(m, text, keep, n_lines, out, out_cap, kept_bytes, total_bytes, Z); }
        }
        if (!found && keep) return fail(ctx, HPGV_ERR_STATE, "no hpgv_filter_text call holds this text");
        return rc;
    }
    if (!ctx) return HPGV_ERR_INVALID;
    hpgv_ctx::TextHeld h;
    if (!take_held(ctx, text, &h)) return keep ? fail(ctx, HPGV_ERR_STATE, "no hpgv_filter_text call holds this text") : HPGV_OK;
    DeviceGuard g(ctx->device);
    SlotLease lease(ctx);
    lease.s = h.slot;                                               // handed back whatever happens below
    if (!keep) return HPGV_OK;                                      // only the hold released
    Slot *s = h.slot;
    if (n_lines != h.n_lines) return fail(ctx, HPGV_ERR_INVALID, "n_lines %d, but hpgv_filter_text tokenized %d lines", n_lines, h.n_lines);
    if (Z && Z->comp) Z->comp[0] = Z->comp[1] = 0;
    if (Z && Z->last) Z->last[0] = Z->last[1] = '\n';
    if (n_lines == 0) { if (kept_bytes) *kept_bytes = 0; if (total_bytes) *total_bytes = 0; return HPGV_OK; }
    unsigned long long ends[2];
    HIPCHK(ctx, hipMemcpyAsync(&ends[0], h.d_line_off, sizeof ends[0], hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(&ends[1], h.d_line_off + n_lines, sizeof ends[1], hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    const size_t total = (size_t)(ends[1] - ends[0]);
    if (!out || (!Z && total > out_cap)) return fail(ctx, HPGV_ERR_INVALID, "the lines take %zu bytes, out has room for %zu", total, out_cap);
    const size_t n = (size_t)n_lines, scratch = hpgv_lines_partition_scratch_bytes(n_lines);
    const size_t off_keep = round_up(scratch + sizeof(unsigned long long), 256), off_seg = round_up(off_keep + n, 256);
    int rc;
    HIPCHK(ctx, s->aux.reserve_slack(off_seg + 64 + 16));
    HIPCHK(ctx, s->parts.reserve_slack(total + 16));
    char *d_aux = s->aux.as<char>();
    unsigned long long *d_kept = (unsigned long long *)(d_aux + scratch);
    uint8_t *d_keep = (uint8_t *)d_aux + off_keep;
    HIPCHK(ctx, hipMemcpyAsync(d_keep, keep, n, hipMemcpyHostToDevice, s->stream));
    if ((rc = partition_launch(ctx, h.d_text, h.d_line_off, n_lines, d_keep, s->parts.as<char>(), d_kept, d_aux, s->stream))) return rc;
    unsigned long long kept = 0;
    HIPCHK(ctx, hipMemcpyAsync(&kept, d_kept, sizeof kept, hipMemcpyDeviceToHost, s->stream));
    if (Z) {                                                        // seg_off[3] | seg_out_off[3], last[2]
        unsigned long long *d_seg = (unsigned long long *)(d_aux + off_seg), res[4] = {0, 0, 0, 0};
        hipLaunchKernelGGL(k_part_segs, dim3(1), dim3(64), 0, s->stream, (const unsigned long long *)d_kept, (unsigned long long)total, Z->want_rest, d_seg);
        if ((rc = deflate_parts(ctx, s, total, d_seg, 2, d_seg + 3))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(res, d_seg + 3, sizeof res, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        const size_t made = (size_t)res[2];
        if (made > out_cap) return fail(ctx, HPGV_ERR_INVALID, "the members take %zu bytes, out has room for %zu", made, out_cap);
        if (made) HIPCHK(ctx, hipMemcpyAsync(out, s->members.p, made, hipMemcpyDeviceToHost, s->stream));
        if (Z->comp) { Z->comp[0] = res[1]; Z->comp[1] = res[2] - res[1]; }
        if (Z->last) memcpy(Z->last, &res[3], 2);
    } else if (total) HIPCHK(ctx, hipMemcpyAsync(out, s->parts.p, total, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    if (kept_bytes) *kept_bytes = kept;
    if (total_bytes) *total_bytes = total;
    return HPGV_OK;
    }
}

int hpgv_text_partition(hpgv_ctx *ctx, const char *text, const uint8_t *keep, int n_lines, char *out, size_t out_cap,
                        uint64_t *kept_bytes, uint64_t *total_bytes) {
    HPGV_ABI_TRY
    return text_partition(ctx, text, keep, n_lines, out, out_cap, kept_bytes, total_bytes, nullptr);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_text_partition_bgzf(hpgv_ctx *ctx, const char *text, const uint8_t *keep, int n_lines, uint8_t *out, size_t out_cap, int want_rest,
                             uint64_t *kept_bytes, uint64_t *total_bytes, uint64_t *comp_bytes, uint8_t *last_byte) {
    HPGV_ABI_TRY
    BgzfWant Z;
    Z.want_rest = want_rest ? 1 : 0; Z.comp = comp_bytes; Z.last = last_byte;
    return text_partition(ctx, text, keep, n_lines, (char *)out, out_cap, kept_bytes, total_bytes, &Z);
    HPGV_ABI_CATCH(ctx)
}

/* ---- multi-way stable partition of lines: bucket 0's lines, then bucket 1's, ... (hpg-var-vcf split: one file per bucket) ---- */

// entries of the [bucket][tile] matrix the scan runs over; 0 when they do not fit its int index
static size_t msplit_entries(int n_lines, int n_buckets) {
    const size_t e = (size_t)n_buckets * (((size_t)n_lines + 63) / 64);
    return e >= (size_t)INT_MAX ? 0 : e;
}
// scratch: in_tile[n_lines], tile_sum[E], tile_base[E + 1], the scan's block sums
size_t hpgv_lines_multisplit_scratch_bytes(int n_lines, int n_buckets) {
    if (n_lines <= 0 || n_buckets < 1 || n_buckets > 256) return 0;
    const size_t e = msplit_entries(n_lines, n_buckets);
    return ((size_t)n_lines + 2 * e + 1 + (e + 1023) / 1024) * sizeof(unsigned long long);
}

static int multisplit_launch(hpgv_ctx *ctx, const char *d_text, const unsigned long long *d_line_off, int n_lines,
                             const uint8_t *d_bucket, int n_buckets, char *d_out, unsigned long long *d_bucket_off, void *d_scratch,
                             hipStream_t st) {
    if (n_lines == 0) {
        HIPCHK(ctx, hipMemsetAsync(d_bucket_off, 0, sizeof(unsigned long long) * ((size_t)n_buckets + 1), st));
        return HPGV_OK;
    }
    const int n_tiles = (n_lines + 63) / 64, e = (int)msplit_entries(n_lines, n_buckets), hb = (e + 1023) / 1024;
    unsigned long long *in_tile = (unsigned long long *)d_scratch, *tile_sum = in_tile + n_lines, *tile_base = tile_sum + e,
                       *block = tile_base + (size_t)e + 1;
    hipLaunchKernelGGL(hpgv::k_msplit_tile_sums, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, st, d_line_off, d_bucket, n_lines,
                       n_buckets, n_tiles, tile_sum, in_tile);
    hipLaunchKernelGGL(hpgv::k_mtile_sums, dim3((unsigned)hb), dim3(1024), 0, st, (const unsigned long long *)tile_sum, e, block);
    hipLaunchKernelGGL(hpgv::k_head_bases, dim3(1), dim3(1024), 0, st, block, hb);
    hipLaunchKernelGGL(hpgv::k_mtile_offsets, dim3((unsigned)hb), dim3(1024), 0, st, (const unsigned long long *)tile_sum, e,
                       (const unsigned long long *)block, tile_base);
    const long cap = 8L * (ctx->n_cus > 0 ? ctx->n_cus : 256);     // the grid of k_part_copy
    const long blocks = std::min<long>(((long)n_lines + 3) / 4, cap);
    hipLaunchKernelGGL(hpgv::k_msplit_copy, dim3((unsigned)blocks), dim3(256), 0, st, d_text, d_line_off, n_lines, d_bucket, n_buckets,
                       n_tiles, (const unsigned long long *)tile_base, (const unsigned long long *)in_tile, d_out, d_bucket_off);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_lines_multisplit_dev(hpgv_ctx *ctx, const char *d_text, const uint64_t *d_line_off, int n_lines, const uint8_t *d_bucket,
                              int n_buckets, char *d_out, uint64_t *d_bucket_off, void *d_scratch, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_lines < 0 || n_buckets < 1 || n_buckets > 256 || !d_bucket_off ||
        (n_lines > 0 && (!d_text || !d_line_off || !d_bucket || !d_out || !d_scratch)))
        return fail(ctx, HPGV_ERR_INVALID, "bad lines_multisplit_dev arguments");
    if (n_lines > 0 && !msplit_entries(n_lines, n_buckets))
        return fail(ctx, HPGV_ERR_INVALID, "%d lines in %d buckets: more than INT_MAX (bucket, tile) sums", n_lines, n_buckets);
    DeviceGuard g(ctx->device);
    return multisplit_launch(ctx, d_text, (const unsigned long long *)d_line_off, n_lines, d_bucket, n_buckets, d_out,
                             (unsigned long long *)d_bucket_off, d_scratch, (hipStream_t)stream);
    HPGV_ABI_CATCH(ctx)
}

// a copy of the hold hpgv_filter_text left on `host_text` (it stays in the list), or false
static bool peek_held(hpgv_ctx *ctx, const char *host_text, hpgv_ctx::TextHeld *out) {
    std::lock_guard<std::mutex> lk(ctx->alias_mu);
    for (const auto &h : ctx->text_held) if (h.host_text == host_text) { *out = h; return true; }
    return false;
}

static int text_multisplit(hpgv_ctx *ctx, const char *text, const uint8_t *bucket, int first_line, int n_lines, int n_buckets,
                           char *out, size_t out_cap, uint64_t *bucket_off, const BgzfWant *Z) {
    {
    if (is_group(ctx)) {
        hpgv_ctx::TextHeld h;
        for (hpgv_ctx *m : ctx->members)
            if (peek_held(m, text, &h)) return text_multisplit(m, text, bucket, first_line, n_lines, n_buckets, out, out_cap, bucket_off, Z);
        return fail(ctx, HPGV_ERR_STATE, "no hpgv_filter_text call holds this text");
    }
    if (!ctx) return HPGV_ERR_INVALID;
    hpgv_ctx::TextHeld h;
    if (!peek_held(ctx, text, &h)) return fail(ctx, HPGV_ERR_STATE, "no hpgv_filter_text call holds this text");
    if (first_line < 0 || n_lines < 0 || first_line > h.n_lines || n_lines > h.n_lines - first_line)
        return fail(ctx, HPGV_ERR_INVALID, "lines [%d, %d + %d), but hpgv_filter_text tokenized %d lines", first_line, first_line, n_lines, h.n_lines);
    if (n_buckets < 1 || n_buckets > 256 || !bucket_off || (n_lines > 0 && !bucket))
        return fail(ctx, HPGV_ERR_INVALID, "bad text_multisplit arguments");
    if (Z && Z->last) memset(Z->last, '\n', (size_t)n_buckets);
    if (n_lines == 0) { memset(bucket_off, 0, sizeof(uint64_t) * ((size_t)n_buckets + 1)); return HPGV_OK; }
    if (!msplit_entries(n_lines, n_buckets))
        return fail(ctx, HPGV_ERR_INVALID, "%d lines in %d buckets: more than INT_MAX (bucket, tile) sums", n_lines, n_buckets);
    DeviceGuard g(ctx->device);
    Slot *s = h.slot;                                               // leased to the hold, which this call keeps
    const unsigned long long *d_line_off = h.d_line_off + first_line;
    unsigned long long ends[2];
    HIPCHK(ctx, hipMemcpyAsync(&ends[0], d_line_off, sizeof ends[0], hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(&ends[1], d_line_off + n_lines, sizeof ends[1], hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    const size_t total = (size_t)(ends[1] - ends[0]), n = (size_t)n_lines, nb1 = (size_t)n_buckets + 1;
    const size_t scratch = hpgv_lines_multisplit_scratch_bytes(n_lines, n_buckets);
    // bucket_off[nb1] | the members' offsets [nb1], the parts' last bytes | bucket
    const size_t off_boff = round_up(scratch, 256), off_bucket = round_up(off_boff + (2 * nb1 + 33) * sizeof(unsigned long long), 256);
    int rc;
    HIPCHK(ctx, s->aux.reserve_slack(off_bucket + n + 16));
    HIPCHK(ctx, s->parts.reserve_slack(total + 16));
    char *d_aux = s->aux.as<char>();
    unsigned long long *d_boff = (unsigned long long *)(d_aux + off_boff);
    uint8_t *d_bucket = (uint8_t *)d_aux + off_bucket;
    HIPCHK(ctx, hipMemcpyAsync(d_bucket, bucket, n, hipMemcpyHostToDevice, s->stream));
    if ((rc = multisplit_launch(ctx, h.d_text, d_line_off, n_lines, d_bucket, n_buckets, s->parts.as<char>(), d_boff, d_aux, s->stream))) return rc;
    if (Z) {
        if ((rc = deflate_parts(ctx, s, total, d_boff, n_buckets, d_boff + nb1))) return rc;
        std::vector<uint64_t> res(nb1 + 33);
        HIPCHK(ctx, hipMemcpyAsync(res.data(), d_boff + nb1, nb1 * sizeof(uint64_t) + (size_t)n_buckets, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        const size_t made = (size_t)res[n_buckets];
        if (made > out_cap || (made && !out)) return fail(ctx, HPGV_ERR_INVALID, "the members take %zu bytes, out has room for %zu", made, out_cap);
        memcpy(bucket_off, res.data(), nb1 * sizeof(uint64_t));
        if (Z->last) memcpy(Z->last, res.data() + nb1, (size_t)n_buckets);
        if (made) {
            HIPCHK(ctx, hipMemcpyAsync(out, s->members.p, made, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(ctx, hipStreamSynchronize(s->stream));
        }
        return HPGV_OK;
    }
    HIPCHK(ctx, hipMemcpyAsync(bucket_off, d_boff, nb1 * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    const size_t stored = (size_t)bucket_off[n_buckets];
    if (stored > out_cap || (stored && !out)) return fail(ctx, HPGV_ERR_INVALID, "the lines take %zu bytes, out has room for %zu", stored, out_cap);
    if (stored) {
        HIPCHK(ctx, hipMemcpyAsync(out, s->parts.p, stored, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
    }
    return HPGV_OK;
    }
}

int hpgv_text_multisplit(hpgv_ctx *ctx, const char *text, const uint8_t *bucket, int first_line, int n_lines, int n_buckets,
                         char *out, size_t out_cap, uint64_t *bucket_off) {
    HPGV_ABI_TRY
    return text_multisplit(ctx, text, bucket, first_line, n_lines, n_buckets, out, out_cap, bucket_off, nullptr);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_text_multisplit_bgzf(hpgv_ctx *ctx, const char *text, const uint8_t *bucket, int first_line, int n_lines, int n_buckets,
                              uint8_t *out, size_t out_cap, uint64_t *bucket_off, uint8_t *last_byte) {
    HPGV_ABI_TRY
    BgzfWant Z;
    Z.last = last_byte;
    return text_multisplit(ctx, text, bucket, first_line, n_lines, n_buckets, (char *)out, out_cap, bucket_off, &Z);
    HPGV_ABI_CATCH(ctx)
}

}  // extern "C"
