// hpgv_text_capi.hip -- the front half of every entry point that takes VCF text (include/hpgv.h): the tokenizer's launcher
// (hpgv_tokenize_dev) and its host twin (hpgv_tokenize), the record filters' settings, and text_front -- text to the device,
// tokenize, line heads of an aliased text, record filters, layout -- which hands a Staged to the tools' back halves in
// hpgv_tool_capi.hip and to hpgv_filter_text in hpgv_lines_capi.hip; text_front_skip adds the skip byte per line that the
// permutation and LD kernels read (hpgv_perm_capi.hip, hpgv_ld_capi.hip).
#include "hpgv_internal.h"
#include "hpgv_text_kernels.h"
#include "hpgv_text2_kernels.h"
#include "hpgv_inherit_kernels.h"
#include "hpgv_rows_kernels.h"

extern "C" {

// (hpgv_inflate_blocks_dev: hpgv_inflate_capi.hip)

int hpgv_tokenize_dev(hpgv_ctx *ctx, const char *d_text, size_t text_bytes, int n_samples, int strict,
                      int max_lines, int *d_n_lines, uint64_t *d_line_off, uint32_t *d_field_off,
                      uint8_t *d_gt, size_t pitch, uint8_t *d_is_x, int32_t *d_status, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_samples < 0 || max_lines < 0 || !d_n_lines || (text_bytes > 0 && !d_text) ||
        (max_lines > 0 && !d_gt) || pitch < (size_t)n_samples)
        return fail(ctx, HPGV_ERR_INVALID, "bad tokenize arguments");
    if (text_bytes > ((size_t)1 << 40)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "text buffer too large for one call");
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    // a window of text the bgzip decoder left with its tile records (hpgv_text_alias_tiles): tokenized on the decoder's tile grid,
    // from the start of the tile the window begins in (grid_skip bytes in front of the window: the tail of the line before it)
    hpgv_ctx::TextTiles TT = {nullptr, nullptr, nullptr, 0};
    bool grid = false;
    size_t grid_t0 = 0, grid_skip = 0;
    if (ctx->tokenizer_tiles == 1 && ctx->decode_tiles && text_bytes > 0 && tiles_of_device_text(ctx, d_text, &TT)) {
        const size_t a = (size_t)(d_text - TT.d_base), e = a + text_bytes;
        if ((e - 1) / hpgv::TOK2_TILE < TT.n_tiles) {
            grid = true; grid_t0 = a / hpgv::TOK2_TILE; grid_skip = a - grid_t0 * hpgv::TOK2_TILE;
            d_text -= grid_skip; text_bytes += grid_skip;
        }
    }
    const size_t n_blocks = (text_bytes + hpgv::TOK_TILE - 1) / hpgv::TOK_TILE;
    if (n_blocks > 0x7FFFFFFFu) return fail(ctx, HPGV_ERR_UNSUPPORTED, "text buffer too large for one call");
    hpgv_ctx::TokScratch *ts = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->tok_mu);
        for (auto *t : ctx->tok_scratch) if (t->stream == st) ts = t;
        if (!ts) { ts = new hpgv_ctx::TokScratch(); ts->stream = st; ctx->tok_scratch.push_back(ts); }
    }
    // from here on `ts` is only touched by calls on stream `st`, which the caller does not issue concurrently
    // scratch per tile: the newline counts of the three-sweep form (4 B), or the tile records and tile states of the
    // tile-parallel form (16 B + 16 B)
    const size_t scratch_ints = (n_blocks + 1) * 8 * (hpgv::TOK_TILE / hpgv::TOK2_TILE > 1 ? hpgv::TOK_TILE / hpgv::TOK2_TILE : 1) + 64;            // (+ the one-sweep form's 64-byte head and the records of a text of a few bytes)
    HIPCHK(ctx, ts->blocks.reserve_after_sync(st, scratch_ints * sizeof(int)));      // (a block still in use by the stream's queued work is not freed under it)
    int *d_blocks = ts->blocks.as<int>();
    unsigned long long *line_off = (unsigned long long *)d_line_off;
    if (!line_off) {                                   // caller does not want the offsets: use scratch
        HIPCHK(ctx, ts->line_off.reserve_after_sync(st, ((size_t)max_lines + 2) * sizeof(unsigned long long)));
        line_off = ts->line_off.as<unsigned long long>();
    }
    if (ctx->tokenizer_tiles) {
        // two sweeps of the text: tile records, tile states, then one workgroup per tile parses (hpgv_text2_kernels.h)
        const size_t n_tiles = (text_bytes + hpgv::TOK2_TILE - 1) / hpgv::TOK2_TILE;      // 2 KiB tiles
        hpgv::TokAgg *agg = (hpgv::TokAgg *)d_blocks;
        hpgv::TokPre *pre = (hpgv::TokPre *)(agg + n_tiles + 1);
        const int n_groups = (int)((n_tiles + hpgv::TOK_SCAN_THREADS - 1) / hpgv::TOK_SCAN_THREADS);
        // the groups' totals and the per-line "parse again" flags live behind the line offsets' scratch
        const size_t extra = ((size_t)n_groups + 2) * sizeof(hpgv::TokState) + ((size_t)max_lines + 2) * sizeof(int);
        HIPCHK(ctx, ts->extra.reserve_after_sync(st, extra, extra + extra / 4));
        hpgv::TokState *gtot = ts->extra.as<hpgv::TokState>();
        int *redo = (int *)(gtot + n_groups + 2), *redo_n = redo + max_lines + 1;      // the list of lines to parse again, its length
        const unsigned redo_grid = (unsigned)(max_lines < 1024 ? max_lines : 1024);
#ifdef HPGV_ABLATION
        if (ctx->tokenizer_tiles >= 2 && n_tiles > 0 && max_lines > 0) {
            // ONE sweep: count, scan and parse in one kernel, the segments' start states by look-back (k_tok_parse3).  The
            // records, the ticket and the error flag share the tile scratch (zeroed per call: 16 bytes per 32 KiB of text).
            const size_t n_seg = (text_bytes + hpgv::TOK3_SEG - 1) / hpgv::TOK3_SEG;
            unsigned *tk = (unsigned *)d_blocks;
            int *err = (int *)d_blocks + 1;
            redo_n = (int *)d_blocks + 2;                          // (zeroed with the records)
            const size_t n_sup = (n_seg + hpgv::TOK3_SUPER - 1) / hpgv::TOK3_SUPER;
            hpgv::TokRec *rec = (hpgv::TokRec *)((char *)d_blocks + 64), *sup = rec + n_seg;
            HIPCHK(ctx, hipMemsetAsync(d_blocks, 0, 64 + (n_seg + n_sup) * sizeof(hpgv::TokRec), st));
            hipLaunchKernelGGL(hpgv::k_tok_parse3, dim3((unsigned)n_seg), dim3(256), 0, st, d_text, text_bytes, rec, sup, tk, err, d_n_lines,
                               max_lines, n_samples, strict, d_gt, pitch, d_is_x, line_off, d_field_off, d_status, redo, redo_n);
            hipLaunchKernelGGL(hpgv::k_tok_finish, dim3(1), dim3(1), 0, st, (const int *)err, d_n_lines);
            hipLaunchKernelGGL(hpgv::k_tok_parse_listed, dim3(redo_grid), dim3(256), 0, st, d_text, line_off,
                               (const int *)d_n_lines, max_lines, n_samples, strict, d_gt, pitch, d_is_x, d_field_off, d_status, (const int *)redo, (const int *)redo_n);
            HIPCHK(ctx, hipGetLastError());
            return HPGV_OK;
        }
#endif
        if (grid && n_tiles > 0) {
            // the decoder's records serve every tile but the window's last, which is counted again up to the window's end
            // (and the bytes in front of the window, for the number of lines that end there)
            const size_t lt = n_tiles - 1;
            hipLaunchKernelGGL(hpgv::k_tok_count2, dim3(1), dim3(256), 0, st, d_text + lt * hpgv::TOK2_TILE, text_bytes - lt * hpgv::TOK2_TILE, 1, agg);
            if (grid_skip) hipLaunchKernelGGL(hpgv::k_tok_count2, dim3(1), dim3(256), 0, st, d_text, grid_skip, 1, agg + 1);
            hipLaunchKernelGGL(hpgv::k_tok_scan2a_grid, dim3((unsigned)n_groups), dim3(hpgv::TOK_SCAN_THREADS), 0, st, (const hpgv::TokAgg2 *)TT.d_tiles, (long)grid_t0,
                               (const hpgv::TokAgg *)agg, d_text, text_bytes, (int)n_tiles, pre, gtot);
        } else if (n_tiles > 0) {
            hipLaunchKernelGGL(hpgv::k_tok_count2, dim3((unsigned)((n_tiles + hpgv::TOK2_COUNT_TILES - 1) / hpgv::TOK2_COUNT_TILES)), dim3(256), 0, st, d_text, text_bytes, (int)n_tiles, agg);
            hipLaunchKernelGGL(hpgv::k_tok_scan2a, dim3((unsigned)n_groups), dim3(hpgv::TOK_SCAN_THREADS), 0, st, (const hpgv::TokAgg *)agg, (int)n_tiles, pre, gtot);
        }
        hipLaunchKernelGGL(hpgv::k_tok_scan2b, dim3((unsigned)(n_groups > 0 ? n_groups : 1)), dim3(hpgv::TOK_SCAN_THREADS), 0, st, pre, (int)n_tiles, gtot, n_groups,
                           d_text, text_bytes, d_n_lines, line_off, max_lines, redo_n, grid_skip ? (const hpgv::TokAgg *)(agg + 1) : (const hpgv::TokAgg *)nullptr);
        if (n_tiles > 0 && max_lines > 0) {
            hipLaunchKernelGGL(hpgv::k_tok_parse2, dim3((unsigned)n_tiles), dim3(hpgv::TOK2_THREADS), 0, st, d_text, text_bytes, (const hpgv::TokPre *)pre,
                               max_lines, n_samples, strict, d_gt, pitch, d_is_x, line_off, d_field_off, d_status, redo, redo_n, (int)grid_skip);
            // the lines whose FORMAT does not begin with GT (listed by the thread that read it): once more, line by line
            hipLaunchKernelGGL(hpgv::k_tok_parse_listed, dim3(redo_grid), dim3(256), 0, st, d_text, line_off,
                               (const int *)d_n_lines, max_lines, n_samples, strict, d_gt, pitch, d_is_x, d_field_off, d_status, (const int *)redo, (const int *)redo_n);
        }
        if (grid_skip)                                               // positions counted from the first tile's start: back to the window's
            hipLaunchKernelGGL(hpgv::k_tok_grid_finish, dim3((unsigned)((max_lines + 256) / 256)), dim3(256), 0, st, line_off, (const int *)d_n_lines, max_lines, (unsigned)grid_skip);
        HIPCHK(ctx, hipGetLastError());
        return HPGV_OK;
    }
#ifndef HPGV_ABLATION
    return fail(ctx, HPGV_ERR_UNSUPPORTED, "the line-by-line tokenizer is an ablation build's");
#else
    if (n_blocks > 0)
        hipLaunchKernelGGL(hpgv::k_tok_count, dim3((unsigned)n_blocks), dim3(256), 0, st, d_text, text_bytes, d_blocks);
    hipLaunchKernelGGL(hpgv::k_tok_scan, dim3(1), dim3(hpgv::TOK_SCAN_THREADS), 0, st, d_blocks, (int)n_blocks, d_text, text_bytes,
                       d_n_lines, line_off, max_lines);
    if (n_blocks > 0)
        hipLaunchKernelGGL(hpgv::k_tok_mark, dim3((unsigned)n_blocks), dim3(256), 0, st, d_text, text_bytes,
                           (const int *)d_blocks, line_off, max_lines);
    else
        HIPCHK(ctx, hipMemsetAsync(line_off, 0, sizeof(unsigned long long), st));
    if (max_lines > 0)
        hipLaunchKernelGGL(hpgv::k_tok_parse, dim3((unsigned)max_lines), dim3(256), 0, st, d_text, line_off,
                           (const int *)d_n_lines, max_lines, n_samples, strict, d_gt, pitch, d_is_x, d_field_off, d_status);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
#endif
    HPGV_ABI_CATCH(ctx)
}

}  // extern "C"

namespace {

// stage 1 of a text call: the text on the device -- where hpgv_text_alias says it lies already (use_alias), else uploaded into
// the slot's `text` -- and tokenized into the slot's raw / isx / status / meta; *n_lines is on the host when this returns.
// *d_text: where the text lies
int tokenize_text(hpgv_ctx *ctx, Slot *s, const char *text, size_t text_bytes, bool use_alias, int n_samples, int strict, int max_lines,
                  size_t raw_pitch, int *n_lines, const char **d_text) {
    const size_t ml = (size_t)max_lines;
    HIPCHK(ctx, s->text.reserve_slack(text_bytes + 16));
    HIPCHK(ctx, s->raw.reserve_slack(ml * raw_pitch + 16));
    HIPCHK(ctx, s->isx.reserve_slack(ml + 16));
    HIPCHK(ctx, s->status.reserve_slack(ml * sizeof(int32_t) + 16));
    HIPCHK(ctx, s->meta.reserve_slack(TextMeta::bytes(max_lines)));
    const TextMeta M(s->meta, max_lines);
    const char *d_src = use_alias ? text_on_device(ctx, text) : nullptr;
    if (!d_src) {
        if (text_bytes) HIPCHK(ctx, hipMemcpyAsync(s->text.p, text, text_bytes, hipMemcpyHostToDevice, s->stream));
        d_src = s->text.as<char>();
    }
    *d_text = d_src;
    for (int attempt = 0; ; ++attempt) {
        if (const int rc = hpgv_tokenize_dev(ctx, d_src, text_bytes, n_samples, strict, max_lines, M.n_lines(), (uint64_t *)M.line_off(), M.field_off(),
                                             s->raw.as<uint8_t>(), raw_pitch, s->isx.as<uint8_t>(), s->status.as<int32_t>(), s->stream)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(n_lines, M.n_lines(), sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        if (*n_lines >= 0 || attempt) return HPGV_OK;
        ctx->tokenizer_tiles = 1;                                    // the one-sweep tokenizer gave up a look-back: the two-sweep kernels from now on
    }
}

// stage 2, for a text that is on the device only: the caller's host buffer gets the line heads (CHROM .. FORMAT, all it reads for
// its result records) and line_off refers to them
int heads_to_host(hpgv_ctx *ctx, Slot *s, const TextMeta &M, int nl, const char *d_src, const char *text, size_t text_bytes, uint64_t *line_off) {
    const int hb = (nl + 1023) / 1024;                              // workgroups of 1024 lines
    const size_t off_heads = (((size_t)nl + 2 + (size_t)hb + 1) * sizeof(uint64_t) + 15) / 16 * 16;
    HIPCHK(ctx, s->heads.reserve_slack(text_bytes + off_heads + 64));
    unsigned long long *d_head_off = s->heads.as<unsigned long long>(), *d_block = d_head_off + (size_t)nl + 2;
    char *d_heads = s->heads.as<char>() + off_heads;
    hipLaunchKernelGGL(hpgv::k_head_sums, dim3((unsigned)hb), dim3(1024), 0, s->stream, (const unsigned long long *)M.line_off(),
                       (const uint32_t *)M.field_off(), nl, d_block);
    hipLaunchKernelGGL(hpgv::k_head_bases, dim3(1), dim3(1024), 0, s->stream, d_block, hb);
    hipLaunchKernelGGL(hpgv::k_head_offsets, dim3((unsigned)hb), dim3(1024), 0, s->stream, (const unsigned long long *)M.line_off(),
                       (const uint32_t *)M.field_off(), nl, (const unsigned long long *)d_block, d_head_off);
    hipLaunchKernelGGL(hpgv::k_copy_heads, dim3((unsigned)nl), dim3(64), 0, s->stream, d_src, (const unsigned long long *)M.line_off(),
                       (const unsigned long long *)d_head_off, nl, d_heads);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long total_heads = 0;
    HIPCHK(ctx, hipMemcpyAsync(&total_heads, d_head_off + nl, sizeof total_heads, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    if (total_heads > text_bytes) return fail(ctx, HPGV_ERR_HIP, "line heads longer than the text");
    if (total_heads) HIPCHK(ctx, hipMemcpyAsync(const_cast<char *>(text), d_heads, (size_t)total_heads, hipMemcpyDeviceToHost, s->stream));
    if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, d_head_off, ((size_t)nl + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    return HPGV_OK;
}

// one record filter over the staged raw matrix: laid out as `which` (Lf; `need` says what sets it), scanned -- scan(rows, &verdicts)
// queues the filter's kernels and says where their verdicts lie -- and `bytes` of verdicts queued back into `out`.  `laid` is kept
// large enough for the tool's own layout (tool_pitch), which comes last
template <typename Scan>
int filter_pass(hpgv_ctx *ctx, Slot *s, const Staged &S, int n_samples, size_t tool_pitch, int which, const Layout &Lf, const char *need, Scan &&scan,
                void *out, size_t bytes) {
    if (!Lf.set || Lf.n_samples != n_samples) return fail(ctx, HPGV_ERR_STATE, need, n_samples);
    HIPCHK(ctx, s->laid.reserve_slack((size_t)S.n * std::max(Lf.pitch, tool_pitch) + 16));
    if (const int rc = hpgv_layout_dev(ctx, which, S.d_raw, S.raw_pitch, S.n, s->laid.as<uint8_t>(), s->stream)) return rc;
    const void *d_verdict = nullptr;
    if (const int rc = scan(s->laid.as<const uint8_t>(), &d_verdict)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, d_verdict, bytes, hipMemcpyDeviceToHost, s->stream));
    return HPGV_OK;
}

// stage 3: the record filters (--maf, --missing, --mendel, --inh-dom, --inh-rec: shared_options.c:44-56,101-173), each from the same
// raw matrix; a rejected line gets HPGV_LINE_FILTERED in the caller's status
int record_filters(hpgv_ctx *ctx, Slot *s, const Staged &S, const Layout &L, int32_t *status) {
    const bool f_counts = ctx->filt_min_maf >= 0.0 || ctx->filt_max_missing >= 0.0, f_mendel = ctx->filt_max_mendel >= 0;
    const bool f_inh = ctx->filt_min_dom >= 0.0 || ctx->filt_min_rec >= 0.0;
    if (!f_counts && !f_mendel && !f_inh) return HPGV_OK;
    int rc;
    const int nl = S.n;
    const size_t n = (size_t)nl;
    std::vector<uint8_t> keep(f_counts ? n : 0), ikeep(f_inh ? n : 0);
    std::vector<int32_t> merr(f_mendel ? n : 0);
    if (f_inh && (rc = filter_pass(ctx, s, S, L.n_samples, L.pitch, HPGV_LAYOUT_ASSOC, ctx->assoc, "the inheritance filters need hpgv_set_cohort over %d columns",
                                   [&](const uint8_t *d_gt, const void **d_verdict) {
        HIPCHK(ctx, s->inherit.reserve_slack(n * 33 + 64));
        int32_t *d_c8 = s->inherit.as<int32_t>();
        uint8_t *d_ikeep = s->inherit.as<uint8_t>() + n * 32;
        if (const int e = hpgv_inheritance_scan_dev(ctx, d_gt, nl, d_c8, s->stream)) return e;
        hipLaunchKernelGGL(hpgv::k_inherit_filter, dim3((nl + 255) / 256), dim3(256), 0, s->stream, (const int4 *)d_c8, nl,
                           ctx->filt_min_dom, ctx->filt_min_rec, d_ikeep);
        HIPCHK(ctx, hipGetLastError());
        *d_verdict = d_ikeep;
        return (int)HPGV_OK;
    }, ikeep.data(), n))) return rc;
    if (f_counts && (rc = filter_pass(ctx, s, S, L.n_samples, L.pitch, HPGV_LAYOUT_STATS, ctx->stats, "the count filters need hpgv_set_stats_cohort(%d)",
                                      [&](const uint8_t *d_gt, const void **d_verdict) {
        HIPCHK(ctx, s->tally.reserve_slack(n * 33 + 64));
        int32_t *d_c8 = s->tally.as<int32_t>();
        uint8_t *d_keep = s->tally.as<uint8_t>() + n * 32;
        if (const int e = hpgv_stats_scan_dev(ctx, d_gt, nl, d_c8, s->stream)) return e;
        *d_verdict = d_keep;
        return hpgv_stats_filter_dev(ctx, d_c8, nl, ctx->filt_min_maf, -1.0, ctx->filt_max_missing, d_keep, s->stream);
    }, keep.data(), n))) return rc;
    if (f_mendel && (rc = filter_pass(ctx, s, S, L.n_samples, L.pitch, HPGV_LAYOUT_MENDEL, ctx->mendel, "the Mendelian error filter needs hpgv_set_pedigree over %d columns",
                                      [&](const uint8_t *d_gt, const void **d_verdict) {
        HIPCHK(ctx, s->merr.reserve_slack(n * sizeof(int32_t) + 64));
        *d_verdict = s->merr.p;
        return hpgv_mendel_scan_dev(ctx, d_gt, nl, S.d_isx, s->merr.as<int32_t>(), s->stream);
    }, merr.data(), n * sizeof(int32_t)))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < n; ++i) {
        const bool out = (f_counts && !keep[i]) || (f_mendel && (long)merr[i] > ctx->filt_max_mendel) || (f_inh && !ikeep[i]);
        if (out) status[i] |= HPGV_LINE_FILTERED;
    }
    return HPGV_OK;
}

}  // namespace

// the raw matrix keeps half-called genotypes ("./1"): the record filters count alleles as the stats tool does; the strict layouts
// (assoc, tdt, epi) turn every not fully called genotype into "missing" on their way in
int text_front(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const char *text, size_t text_bytes,
               int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off, int32_t *status,
               Staged *S, bool final_layout) {
    int rc;
    const size_t raw_pitch = raw_pitch_of(L.n_samples);
    const char *d_src = nullptr;
    HIPCHK(ctx, s->laid.reserve_slack((size_t)max_lines * L.pitch + 16));
    if ((rc = tokenize_text(ctx, s, text, text_bytes, true, L.n_samples, 0, max_lines, raw_pitch, n_lines, &d_src))) return rc;
    const TextMeta M(s->meta, max_lines);
    const int nl = *n_lines < max_lines ? *n_lines : max_lines;
    S->text = true;
    S->d_raw = s->raw.as<uint8_t>(); S->raw_pitch = raw_pitch; S->d_isx = s->isx.as<uint8_t>();
    S->n = nl; S->out_stride = (size_t)max_lines;
    if (nl == 0) return HPGV_OK;
    if (status) HIPCHK(ctx, hipMemcpyAsync(status, s->status.p, (size_t)nl * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (d_src != s->text.p) {
        if ((rc = heads_to_host(ctx, s, M, nl, d_src, text, text_bytes, line_off))) return rc;
    } else if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, M.line_off(), ((size_t)nl + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    if (field_off) HIPCHK(ctx, hipMemcpyAsync(field_off, M.field_off(), (size_t)nl * 10 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    if (status && (rc = record_filters(ctx, s, *S, L, status))) return rc;
    if (!final_layout) return HPGV_OK;                       // the caller's one-pass kernel reads the raw matrix itself
    S->d_laid = s->laid.as<uint8_t>(); S->which = which;
    return hpgv_layout_dev(ctx, which, S->d_raw, raw_pitch, nl, s->laid.as<uint8_t>(), s->stream);
}

// the lines a caller of the plain *_text entry points drops: not a record (status 1), or rejected by a record filter
static bool line_skipped(int32_t status) { return (status & 0xFF) == 1 || (status & HPGV_LINE_FILTERED); }

// the record filters run only into a status array, so the call brings its own when the caller gave none
int text_front_skip(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                    uint64_t *line_off, uint32_t *field_off, int32_t *status, TextSkip *K, Staged *S, bool final_layout) {
    if (!status) { K->own_status.assign((size_t)max_lines, 0); status = K->own_status.data(); }
    if (const int rc = text_front(ctx, s, which, L, text, text_bytes, max_lines, n_lines, line_off, field_off, status, S, final_layout)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    K->skip.resize((size_t)S->n);
    for (int i = 0; i < S->n; ++i) K->skip[(size_t)i] = line_skipped(status[i]) ? 1 : 0;
    return HPGV_OK;
}

namespace {

// scratch of the gather: dst_row[n_rows + 1], then the scan's block sums
size_t rows_scratch_bytes(int n_rows) { return ((size_t)n_rows + 1 + ((size_t)n_rows + 1023) / 1024 + 1) * sizeof(uint64_t); }

// dst_row = the exclusive scan of the flags (n_rows > 0)
int rows_scan(hpgv_ctx *ctx, const uint8_t *d_keep, int n_rows, unsigned long long *d_dst_row, hipStream_t st) {
    const int hb = (n_rows + 1023) / 1024;
    unsigned long long *d_block = d_dst_row + (size_t)n_rows + 1;
    hipLaunchKernelGGL(hpgv::k_rows_kept_sums, dim3((unsigned)hb), dim3(1024), 0, st, d_keep, n_rows, d_block);
    hipLaunchKernelGGL(hpgv::k_head_bases, dim3(1), dim3(1024), 0, st, d_block, hb);
    hipLaunchKernelGGL(hpgv::k_rows_kept_offsets, dim3((unsigned)hb), dim3(1024), 0, st, d_keep, n_rows, (const unsigned long long *)d_block, d_dst_row);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

// the kept rows to their places, the index array and the count (n_rows > 0, after rows_scan on the same stream)
int rows_copy(hpgv_ctx *ctx, const uint8_t *d_src, size_t src_pitch, size_t row_bytes, int n_rows, const uint8_t *d_keep,
              const unsigned long long *d_dst_row, uint8_t *d_dst, size_t dst_pitch, int32_t *d_index, int32_t *d_n_kept, hipStream_t st) {
    const bool aligned = ((src_pitch | dst_pitch | (uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0;
    int T = 1;
    while (T < 64 && 16ull * (unsigned long long)T < row_bytes) T <<= 1;
    const long long waves = ((long long)n_rows + 64 / T - 1) / (64 / T);
    long long wgs = (waves + 3) / 4;
    const long long most = (long long)ctx->n_cus * 8;
    wgs = wgs < 1 ? 1 : (wgs > most ? most : wgs);
    if (aligned)
        hipLaunchKernelGGL(hpgv::k_rows_copy<true>, dim3((unsigned)wgs), dim3(256), 0, st, d_src, src_pitch, row_bytes, n_rows, d_keep, d_dst_row,
                           d_dst, dst_pitch, d_index, d_n_kept);
    else
        hipLaunchKernelGGL(hpgv::k_rows_copy<false>, dim3((unsigned)wgs), dim3(256), 0, st, d_src, src_pitch, row_bytes, n_rows, d_keep, d_dst_row,
                           d_dst, dst_pitch, d_index, d_n_kept);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

}  // namespace

// the back half of hpgv_assoc_select_text (hpgv_tool_capi.hip), once the tool's results are out and the stream is idle: flags from
// the statuses (the caller's, with the record filters' verdicts in them) and the device p-values, the scan, and -- when they fit
// rows_cap -- the candidate rows of the slot's raw matrix, compacted on the device, into rows_out
int select_rows(hpgv_ctx *ctx, Slot *s, const Staged &S, int n_samples, const int32_t *status, const char *d_p, size_t p_stride, double p_max,
                int32_t *sel, uint8_t *rows_out, size_t rows_pitch, int rows_cap, int *n_sel) {
    int rc;
    const int nl = S.n;
    const size_t n = (size_t)nl, off_index = round_up(n, 16), off_count = off_index + n * sizeof(int32_t), off_scan = round_up(off_count + 4, 16);
    HIPCHK(ctx, s->perm.reserve_slack(off_scan + rows_scratch_bytes(nl) + 16));
    uint8_t *d_keep = s->perm.as<uint8_t>();
    int32_t *d_index = (int32_t *)(s->perm.as<char>() + off_index), *d_count = (int32_t *)(s->perm.as<char>() + off_count);
    unsigned long long *d_dst_row = (unsigned long long *)(s->perm.as<char>() + off_scan);
    HIPCHK(ctx, hipMemcpyAsync(s->status.p, status, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(hpgv::k_select_flags, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s->stream, s->status.as<const int32_t>(), d_p, p_stride, nl,
                       p_max, d_keep);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = rows_scan(ctx, d_keep, nl, d_dst_row, s->stream))) return rc;
    unsigned long long kept = 0;
    HIPCHK(ctx, hipMemcpyAsync(&kept, d_dst_row + n, sizeof kept, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    *n_sel = (int)kept;
    // the compact block: the candidates alone, rows a raw pitch apart.  One row of room where there is no candidate or no room in
    // the caller's block: the copy kernel still writes the index array, and stores no row byte then (no flag set, or none wanted)
    const bool fits = (int)kept <= rows_cap;
    const size_t dpitch = S.raw_pitch;
    HIPCHK(ctx, s->gtally.reserve_slack((fits && kept ? (size_t)kept : 1) * dpitch + 16));
    if ((rc = rows_copy(ctx, S.d_raw, S.raw_pitch, fits ? (size_t)n_samples : 0, nl, d_keep, d_dst_row, s->gtally.as<uint8_t>(), fits ? dpitch : 0, d_index,
                        d_count, s->stream))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(sel, d_index, n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (fits && kept && n_samples > 0)
        HIPCHK(ctx, hipMemcpy2DAsync(rows_out, rows_pitch, s->gtally.p, dpitch, (size_t)n_samples, (size_t)kept, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

extern "C" {

size_t hpgv_rows_gather_scratch_bytes(int n_rows) { return n_rows > 0 ? rows_scratch_bytes(n_rows) : 16; }

int hpgv_rows_gather_dev(hpgv_ctx *ctx, const uint8_t *d_src, size_t src_pitch, size_t row_bytes, int n_rows, const uint8_t *d_keep,
                         uint8_t *d_dst, size_t dst_pitch, int32_t *d_index, int32_t *d_n_kept, void *d_scratch, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_rows < 0 || !d_n_kept || (n_rows > 0 && (!d_keep || !d_index || !d_scratch || (row_bytes > 0 && (!d_src || !d_dst)))))
        return fail(ctx, HPGV_ERR_INVALID, "bad rows_gather arguments");
    if (src_pitch < row_bytes || dst_pitch < row_bytes) return fail(ctx, HPGV_ERR_INVALID, "a pitch below row_bytes %zu", row_bytes);
    if (((uintptr_t)d_scratch & 7) || ((uintptr_t)d_index & 3) || ((uintptr_t)d_n_kept & 3))
        return fail(ctx, HPGV_ERR_INVALID, "d_scratch must be 8-byte aligned, d_index and d_n_kept 4-byte aligned");
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) { HIPCHK(ctx, hipMemsetAsync(d_n_kept, 0, sizeof(int32_t), st)); return HPGV_OK; }
    if (const int rc = rows_scan(ctx, d_keep, n_rows, (unsigned long long *)d_scratch, st)) return rc;
    return rows_copy(ctx, d_src, src_pitch, row_bytes, n_rows, d_keep, (const unsigned long long *)d_scratch, d_dst, dst_pitch, d_index, d_n_kept, st);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_tokenize(hpgv_ctx *ctx, const char *text, size_t text_bytes, int n_samples, int strict, int max_lines,
                  int *n_lines, uint64_t *line_off, uint32_t *field_off, uint8_t *gt, size_t pitch,
                  uint8_t *is_x, int32_t *status) {
    GROUP_DEAL(ctx, hpgv_tokenize(m_, text, text_bytes, n_samples, strict, max_lines, n_lines, line_off, field_off, gt, pitch, is_x, status))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!n_lines || n_samples < 0 || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !gt) ||
        pitch < (size_t)n_samples)
        return fail(ctx, HPGV_ERR_INVALID, "bad tokenize arguments");
    HPGV_LEASE_SLOT(ctx)
    const char *d_src = nullptr;
    if ((rc = tokenize_text(ctx, s, text, text_bytes, false, n_samples, strict, max_lines, pitch, n_lines, &d_src))) return rc;
    const TextMeta M(s->meta, max_lines);
    const size_t nl = (size_t)(*n_lines < max_lines ? *n_lines : max_lines);
    if (nl) {
        HIPCHK(ctx, hipMemcpyAsync(gt, s->raw.p, nl * pitch, hipMemcpyDeviceToHost, s->stream));
        if (is_x) HIPCHK(ctx, hipMemcpyAsync(is_x, s->isx.p, nl, hipMemcpyDeviceToHost, s->stream));
        if (field_off) HIPCHK(ctx, hipMemcpyAsync(field_off, M.field_off(), nl * 10 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        if (status) HIPCHK(ctx, hipMemcpyAsync(status, s->status.p, nl * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    }
    if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, M.line_off(), (nl + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

int hpgv_set_text_filters(hpgv_ctx *ctx, double min_maf, double max_missing, long max_mendel_errors) {
    GROUP_ALL(ctx, hpgv_set_text_filters(m_, min_maf, max_missing, max_mendel_errors))
    if (!ctx) return HPGV_ERR_INVALID;
    if (min_maf > 0.5 || max_missing > 1.0) return fail(ctx, HPGV_ERR_INVALID, "min_maf is at most 0.5, max_missing at most 1");
    ctx->filt_min_maf = min_maf; ctx->filt_max_missing = max_missing; ctx->filt_max_mendel = max_mendel_errors;
    return HPGV_OK;
}

int hpgv_set_text_inheritance_filters(hpgv_ctx *ctx, double min_dominant, double min_recessive) {
    GROUP_ALL(ctx, hpgv_set_text_inheritance_filters(m_, min_dominant, min_recessive))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!(min_dominant <= 1.0) || !(min_recessive <= 1.0)) return fail(ctx, HPGV_ERR_INVALID, "the inheritance thresholds are at most 1");
    ctx->filt_min_dom = min_dominant < 0.0 ? -1.0 : min_dominant;
    ctx->filt_min_rec = min_recessive < 0.0 ? -1.0 : min_recessive;
    return HPGV_OK;
}

}  // extern "C"
