// hpgv_ld_capi.hip -- C ABI of the LD band (include/hpgv.h "LD"): the device-resident launches of k_ld_window and k_ld_edges
// (one grid set-up, ld_grid, for both), the synchronous entry points on a host batch and on a text -- staged like every tool's,
// by stage_chain and text_front_skip (hpgv_internal.h) -- and the host-only helpers: r^2 of six counts, clumping of an edge list.
#include "hpgv_internal.h"
#include "hpgv_ld_kernels.h"
#include <algorithm>
#include <cstddef>

namespace {

static_assert(hpgv::LD_MAX_WINDOW == HPGV_LD_MAX_WINDOW, "the kernel's window limit is the header's");

int ld_window_check(const hpgv_ctx *ctx, int window) {
    if (window < 1 || window > hpgv::LD_MAX_WINDOW)
        return fail(ctx, HPGV_ERR_UNSUPPORTED, "window %d: 1 .. %d variants", window, hpgv::LD_MAX_WINDOW);
    return HPGV_OK;
}

// the grid both forms of the band share (k_ld_window "Grid"): the rows and the bounds of the band into A -- its outputs, r2 and
// counts6, are the caller's to set --, the workgroups into *wgs
int ld_grid(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window, const int32_t *d_chrom,
            const uint32_t *d_pos, int64_t max_bp, const uint8_t *d_skip, hpgv::LdArgs *A, unsigned *wgs) {
    A->gt = d_gt; A->pitch = pitch; A->chunks = (int)(pitch / 16); A->n_variants = n_variants; A->b_begin = b_begin; A->window = window;
    A->passes = (63 + window) / 64 + 1;
    A->tiles = (n_variants + hpgv::LD_VT - 1) / hpgv::LD_VT; A->tiles_per_range = (A->tiles + 7) / 8;
    A->chrom = d_chrom; A->pos = d_pos; A->max_bp = max_bp; A->skip = d_skip;
    const size_t n = (size_t)8 * (size_t)A->tiles_per_range * (size_t)A->passes;
    if (n > 0x7FFFFFFFu) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d variants x window %d in one call: give the variants in several", n_variants, window);
    *wgs = (unsigned)n;
    return HPGV_OK;
}

// the launch: the pairs without an earlier row, then the band (the arguments checked, the device current)
int ld_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window, const int32_t *d_chrom,
              const uint32_t *d_pos, int64_t max_bp, const uint8_t *d_skip, double *d_r2, int32_t *d_counts6, hipStream_t st) {
    if (n_variants == b_begin) return HPGV_OK;
    hpgv::LdArgs A;
    unsigned wgs;
    if (const int rc = ld_grid(ctx, d_gt, pitch, n_variants, b_begin, window, d_chrom, d_pos, max_bp, d_skip, &A, &wgs)) return rc;
    A.r2 = d_r2; A.counts6 = d_counts6;
    const int head_end = n_variants < window ? n_variants : window;           // later variants below `window` lack earlier rows
    const size_t head = head_end > b_begin ? (size_t)(head_end - b_begin) * (size_t)window : 0;
    // (option "profile": the two kernels' time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
        if (head) hipLaunchKernelGGL(hpgv::k_ld_head, dim3((unsigned)((head + 255) / 256)), dim3(256), 0, st, b_begin, head_end, window, d_r2, d_counts6);
        hipLaunchKernelGGL(hpgv::k_ld_window, dim3(wgs), dim3(256), 0, st, A);
    });
}

static_assert(sizeof(hpgv_ld_edge) == 16 && offsetof(hpgv_ld_edge, b) == 4 && offsetof(hpgv_ld_edge, r2) == 8, "k_ld_edges stores a record as one uint4");

// the edge form's launch: the counter zeroed on the stream, then the band's grid with the appending epilogue.  No k_ld_head: a
// pair without an earlier row is no edge
int ld_edges_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window, const int32_t *d_chrom,
                    const uint32_t *d_pos, int64_t max_bp, const uint8_t *d_skip, double min_r2, hpgv_ld_edge *d_edges, uint64_t edge_cap,
                    uint64_t *d_n_edges, hipStream_t st) {
    HIPCHK(ctx, hipMemsetAsync(d_n_edges, 0, sizeof(uint64_t), st));
    if (n_variants == b_begin) return HPGV_OK;
    hpgv::LdArgs A;
    unsigned wgs;
    if (const int rc = ld_grid(ctx, d_gt, pitch, n_variants, b_begin, window, d_chrom, d_pos, max_bp, d_skip, &A, &wgs)) return rc;
    A.r2 = nullptr; A.counts6 = nullptr;
    hpgv::LdEdgeOut E;
    E.min_r2 = min_r2; E.edges = reinterpret_cast<uint4 *>(d_edges); E.cap = edge_cap; E.n_edges = (unsigned long long *)d_n_edges;
    return launch_profiled(ctx, st, 1, [&] { hipLaunchKernelGGL(hpgv::k_ld_edges, dim3(wgs), dim3(256), 0, st, A, E); });
}

// the back half of hpgv_ld and hpgv_ld_text: the laid-out matrix of a staged call -> the band -> the caller's arrays.  skip, chrom
// and pos (host, may be null) are copied to the slot
int ld_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, int window, const uint8_t *skip, const int32_t *chrom, const uint32_t *pos, int64_t max_bp,
              double *r2, int32_t *counts6) {
    const int nv = S.n;
    if (nv > 0) {
        const size_t n = (size_t)nv, pairs = n * (size_t)window, off_pos = round_up(n * sizeof(int32_t), 16);
        HIPCHK(ctx, s->dbl.reserve_slack(pairs * sizeof(double) + 16));
        if (counts6) HIPCHK(ctx, s->tally.reserve_slack(pairs * 6 * sizeof(int32_t) + 16));
        if (skip) HIPCHK(ctx, s->perm.reserve_slack(n + 16));
        if (chrom) HIPCHK(ctx, s->ints.reserve_slack(off_pos + n * sizeof(uint32_t) + 16));
        double *d_r2 = s->dbl.as<double>();
        int32_t *d_counts6 = counts6 ? s->tally.as<int32_t>() : nullptr;
        uint8_t *d_skip = skip ? s->perm.as<uint8_t>() : nullptr;
        int32_t *d_chrom = chrom ? s->ints.as<int32_t>() : nullptr;
        uint32_t *d_pos = chrom ? (uint32_t *)(s->ints.as<char>() + off_pos) : nullptr;
        if (skip) HIPCHK(ctx, hipMemcpyAsync(d_skip, skip, n, hipMemcpyHostToDevice, s->stream));
        if (chrom) {
            HIPCHK(ctx, hipMemcpyAsync(d_chrom, chrom, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
            HIPCHK(ctx, hipMemcpyAsync(d_pos, pos, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
        }
        if (const int rc = ld_launch(ctx, S.d_laid, ctx->assoc.pitch, nv, 0, window, d_chrom, d_pos, max_bp, d_skip, d_r2, d_counts6, s->stream)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(r2, d_r2, pairs * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (counts6) HIPCHK(ctx, hipMemcpyAsync(counts6, d_counts6, pairs * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_ld_window_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window,
                       const int32_t *d_chrom, const uint32_t *d_pos, int64_t max_bp, const uint8_t *d_skip,
                       double *d_r2, int32_t *d_counts6, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = ld_window_check(ctx, window)) return rc;
    if (n_variants < 0 || b_begin < 0 || b_begin > n_variants || (n_variants > b_begin && (!d_gt || !d_r2)))
        return fail(ctx, HPGV_ERR_INVALID, "bad ld_window arguments");
    if ((d_chrom == nullptr) != (d_pos == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "d_chrom and d_pos: both or neither");
    if (pitch == 0 || (pitch & 15) || pitch > 0xFFFFFFF0u) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu: a multiple of 16 below 4 GiB", pitch);
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_r2 & 7) || ((uintptr_t)d_counts6 & 7) || ((uintptr_t)d_chrom & 3) || ((uintptr_t)d_pos & 3))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt must be 16-byte aligned, d_r2 and d_counts6 8-byte aligned, d_chrom and d_pos 4-byte aligned");
    DeviceGuard g(ctx->device);
    return ld_launch(ctx, d_gt, pitch, n_variants, b_begin, window, d_chrom, d_pos, max_bp, d_skip, d_r2, d_counts6, (hipStream_t)stream);
}

int hpgv_ld(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int window, const int32_t *chrom, const uint32_t *pos,
            int64_t max_bp, double *r2, int32_t *counts6) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (is_group(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "hpgv_ld on a group context: the members' shards have seams");
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (const int rc0 = ld_window_check(ctx, window)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !r2))) return fail(ctx, HPGV_ERR_INVALID, "bad ld arguments");
    if ((chrom == nullptr) != (pos == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "chrom and pos: both or neither");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    return ld_finish(ctx, s, S, window, nullptr, chrom, pos, max_bp, r2, counts6);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_ld_edges_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int b_begin, int window,
                      const int32_t *d_chrom, const uint32_t *d_pos, int64_t max_bp, const uint8_t *d_skip,
                      double min_r2, hpgv_ld_edge *d_edges, uint64_t edge_cap, uint64_t *d_n_edges, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = ld_window_check(ctx, window)) return rc;
    if (n_variants < 0 || b_begin < 0 || b_begin > n_variants || (n_variants > b_begin && !d_gt) || !d_n_edges || (edge_cap > 0 && !d_edges))
        return fail(ctx, HPGV_ERR_INVALID, "bad ld_edges arguments");
    if (min_r2 != min_r2) return fail(ctx, HPGV_ERR_INVALID, "min_r2 is NaN");
    if ((d_chrom == nullptr) != (d_pos == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "d_chrom and d_pos: both or neither");
    if (pitch == 0 || (pitch & 15) || pitch > 0xFFFFFFF0u) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu: a multiple of 16 below 4 GiB", pitch);
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_edges & 15) || ((uintptr_t)d_n_edges & 7) || ((uintptr_t)d_chrom & 3) || ((uintptr_t)d_pos & 3))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_edges must be 16-byte aligned, d_n_edges 8-byte aligned, d_chrom and d_pos 4-byte aligned");
    DeviceGuard g(ctx->device);
    return ld_edges_launch(ctx, d_gt, pitch, n_variants, b_begin, window, d_chrom, d_pos, max_bp, d_skip, min_r2, d_edges, edge_cap, d_n_edges,
                           (hipStream_t)stream);
}

int hpgv_ld_edges(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int window, const int32_t *chrom, const uint32_t *pos,
                  int64_t max_bp, double min_r2, hpgv_ld_edge *edges, uint64_t edge_cap, uint64_t *n_edges) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (is_group(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "hpgv_ld_edges on a group context: the members' shards have seams");
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (const int rc0 = ld_window_check(ctx, window)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && !gt) || !n_edges || (edge_cap > 0 && !edges)) return fail(ctx, HPGV_ERR_INVALID, "bad ld_edges arguments");
    if (min_r2 != min_r2) return fail(ctx, HPGV_ERR_INVALID, "min_r2 is NaN");
    if ((chrom == nullptr) != (pos == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "chrom and pos: both or neither");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    *n_edges = 0;
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    const size_t n = (size_t)n_variants, off_pos = round_up(n * sizeof(int32_t), 16);
    // no more pairs than the band holds can qualify: the device list need not be longer
    const uint64_t band = (uint64_t)n * (uint64_t)window, cap = edge_cap < band ? edge_cap : band;
    HIPCHK(ctx, s->dbl.reserve_slack(16 + (size_t)cap * sizeof(hpgv_ld_edge)));           // the counter, then the list
    if (chrom) HIPCHK(ctx, s->ints.reserve_slack(off_pos + n * sizeof(uint32_t) + 16));
    int32_t *d_chrom = chrom ? s->ints.as<int32_t>() : nullptr;
    uint32_t *d_pos = chrom ? (uint32_t *)(s->ints.as<char>() + off_pos) : nullptr;
    if (chrom) {
        HIPCHK(ctx, hipMemcpyAsync(d_chrom, chrom, n * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_pos, pos, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    }
    uint64_t *d_count = s->dbl.as<uint64_t>();
    hpgv_ld_edge *d_edges = cap ? (hpgv_ld_edge *)(s->dbl.as<char>() + 16) : nullptr;
    if ((rc = ld_edges_launch(ctx, S.d_laid, ctx->assoc.pitch, n_variants, 0, window, d_chrom, d_pos, max_bp, nullptr, min_r2, d_edges, cap,
                              d_count, s->stream))) return rc;
    uint64_t count = 0;
    HIPCHK(ctx, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    *n_edges = count;
    if (count == 0 || count > edge_cap) return HPGV_OK;
    HIPCHK(ctx, hipMemcpyAsync(edges, d_edges, (size_t)count * sizeof(hpgv_ld_edge), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    std::sort(edges, edges + count, [](const hpgv_ld_edge &x, const hpgv_ld_edge &y) { return x.b != y.b ? x.b < y.b : x.a < y.a; });
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_ld_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off,
                 int32_t *status, int window, double *r2, int32_t *counts6) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (is_group(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "hpgv_ld_text on a group context: the members' shards have seams");
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (const int rc0 = ld_window_check(ctx, window)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !r2)) return fail(ctx, HPGV_ERR_INVALID, "bad ld_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    // the lines hpgv_assoc_text's callers drop keep their slot in the window as skipped rows
    if ((rc = text_front_skip(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S))) return rc;
    return ld_finish(ctx, s, S, window, K.bytes(), nullptr, nullptr, -1, r2, counts6);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only helper: no GPU call, usable without a device ------------------------------------------------------------ */

double hpgv_ld_r2(const int32_t counts6[6]) {
    return hpgv::ld_r2_value(counts6[0], counts6[1], counts6[2], counts6[3], counts6[4], counts6[5]);
}

int hpgv_clump(int n, const double *p, const hpgv_ld_edge *edges, uint64_t n_edges, double p1, int32_t *index_of, int32_t *clump_order,
               int *n_clumps) {
    try {
        if (n < 0 || !n_clumps || (n > 0 && (!p || !index_of)) || (n_edges > 0 && !edges)) return HPGV_ERR_INVALID;
        *n_clumps = 0;
        // the neighbours of every candidate, both directions of every edge: counts, offsets, fill
        std::vector<uint64_t> first((size_t)n + 1, 0);
        for (uint64_t e = 0; e < n_edges; ++e) {
            const int32_t a = edges[e].a, b = edges[e].b;
            if (a < 0 || a >= n || b < 0 || b >= n) return HPGV_ERR_INVALID;
            ++first[(size_t)a + 1]; ++first[(size_t)b + 1];
        }
        for (int i = 0; i < n; ++i) first[(size_t)i + 1] += first[(size_t)i];
        std::vector<int32_t> nb((size_t)(2 * n_edges));
        std::vector<uint64_t> fill(first.begin(), first.end() - 1);
        for (uint64_t e = 0; e < n_edges; ++e) {
            nb[(size_t)fill[(size_t)edges[e].a]++] = edges[e].b;
            nb[(size_t)fill[(size_t)edges[e].b]++] = edges[e].a;
        }
        std::vector<int32_t> order;
        order.reserve((size_t)n);
        for (int i = 0; i < n; ++i) {
            index_of[i] = -1;
            if (p[i] == p[i]) order.push_back(i);                             // (not NaN)
        }
        std::sort(order.begin(), order.end(), [p](int32_t x, int32_t y) { return p[x] != p[y] ? p[x] < p[y] : x < y; });
        int k = 0;
        for (const int32_t i : order) {
            if (p[i] > p1) break;
            if (index_of[i] != -1) continue;                                  // claimed by a stronger one
            index_of[i] = i;
            if (clump_order) clump_order[k] = i;
            ++k;
            for (uint64_t e = first[(size_t)i]; e < first[(size_t)i + 1]; ++e)
                if (index_of[nb[(size_t)e]] == -1) index_of[nb[(size_t)e]] = i;
        }
        *n_clumps = k;
        return HPGV_OK;
    } catch (const std::bad_alloc &) { return HPGV_ERR_NOMEM; }
}

}  // extern "C"
