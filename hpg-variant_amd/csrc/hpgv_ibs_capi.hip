// hpgv_ibs_capi.hip -- C ABI of the sample-relatedness counts (include/hpgv.h "IBS"): the device-resident launches of k_ibs_pairs,
// k_ibs_class_counts and k_ibs_select, the synchronous entry points on a host batch and on a text -- staged like every tool's, by
// stage_chain and text_front_skip (hpgv_internal.h), through the STATS layout: every sample, in VCF order -- and the host-only
// helpers: the terms of a row's class counts, the genome values of a pair's counts.
#include "hpgv_internal.h"
#include "hpgv_ibs_kernels.h"
#include <cstddef>

int ibs_matrix_check(const hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols) {
    if (n_variants < 0 || n_cols < 0 || (size_t)n_cols > pitch) return fail(ctx, HPGV_ERR_INVALID, "bad ibs arguments: %d rows, %d columns, pitch %zu", n_variants, n_cols, pitch);
    if (pitch == 0 || (pitch & 15) || pitch > 0xFFFFFFF0u) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu: a multiple of 16 below 4 GiB", pitch);
    if ((uintptr_t)d_gt & 15) return fail(ctx, HPGV_ERR_INVALID, "d_gt must be 16-byte aligned");
    return HPGV_OK;
}

static int ibs_class_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, int32_t *d_class4, hipStream_t st) {
    hipLaunchKernelGGL(hpgv::k_ibs_class_counts, dim3((unsigned)(((long long)n_variants + 3) / 4)), dim3(256), 0, st, d_gt, pitch, n_variants, n_cols, d_skip,
                       reinterpret_cast<int4 *>(d_class4));
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

// The front of the back halves of hpgv_ibs / hpgv_grm and their text forms (S.n > 0): the matrix of a staged call as the
// kernels over sample COLUMNS read it, the rows' skip bytes on the device, the class counts queued.  The STATS layout holds
// every sample in VCF order, but its bytes are the stats flags and not HPGV8: the kernels read the RAW matrix, which has the
// same columns -- in place where its pitch is a multiple of 16 (a text's always is), else gathered into the slot's `laid` in the
// stats layout's pitch without recoding.  skip (host, may be null) is copied to the slot; x_too: the rows the tokenizer flagged
// as chromosome X are skipped as well; need_skip: the caller's kernels write skip bytes, so they exist even where none is set
int cols_front(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, bool need_skip, ColsFront *F) {
    const int nv = S.n, ns = ctx->stats.n_samples;
    const size_t n = (size_t)nv;
    const uint8_t *d_gt = S.d_raw;
    size_t gt_pitch = S.raw_pitch;
    if ((gt_pitch & 15) || ((uintptr_t)d_gt & 15)) {
        const Layout &L = ctx->stats;
        HIPCHK(ctx, s->laid.reserve_slack(n * L.pitch + 16));
        const long slab = std::max(1L, (1L << 31) / (L.chunks > 0 ? L.chunks : 1));      // (hpgv_layout_dev's launches)
        for (long off = 0; off < nv; off += slab) {
            const int m = (int)std::min(slab, (long)nv - off);
            hipLaunchKernelGGL(hpgv::k_layout, dim3((unsigned)(((long)m * L.chunks + 255) / 256)), dim3(256), 0, s->stream,
                               S.d_raw + (size_t)off * S.raw_pitch, S.raw_pitch, m, L.pitch, L.chunks, L.d_col_of_pos(), 0, (int)hpgv::RECODE_NONE, 0,
                               s->laid.as<uint8_t>() + (size_t)off * L.pitch);
        }
        HIPCHK(ctx, hipGetLastError());
        d_gt = s->laid.as<uint8_t>(); gt_pitch = L.pitch;
    }
    const bool have_skip = skip != nullptr || x_too || need_skip;
    HIPCHK(ctx, s->tally.reserve_slack(n * 16 + 16));
    if (have_skip) HIPCHK(ctx, s->perm.reserve_slack(n + 16));
    int32_t *d_class4 = s->tally.as<int32_t>();
    uint8_t *d_skip = have_skip ? s->perm.as<uint8_t>() : nullptr;
    if (skip) HIPCHK(ctx, hipMemcpyAsync(d_skip, skip, n, hipMemcpyHostToDevice, s->stream));
    else if (have_skip) HIPCHK(ctx, hipMemsetAsync(d_skip, 0, n, s->stream));
    if (x_too) {
        hipLaunchKernelGGL(hpgv::k_ibs_skip_x, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s->stream, d_skip, S.d_isx, nv);
        HIPCHK(ctx, hipGetLastError());
    }
    if (const int rc = ibs_class_launch(ctx, d_gt, gt_pitch, nv, ns, d_skip, d_class4, s->stream)) return rc;
    F->d_gt = d_gt; F->pitch = gt_pitch; F->d_skip = d_skip; F->d_class4 = d_class4;
    return HPGV_OK;
}

namespace {

static_assert(sizeof(hpgv_ibs_counts) == 16, "k_ibs_pairs adds to a record as four int32, k_ibs_select loads it as one int4");
static_assert(sizeof(hpgv_ibs_pair) == 32 && offsetof(hpgv_ibs_pair, j) == 4 && offsetof(hpgv_ibs_pair, c) == 8 && offsetof(hpgv_ibs_pair, pi_hat) == 24,
              "k_ibs_select stores a record as two uint4");

// the launch of k_ibs_pairs (the arguments checked, the device current, rows and pairs to do): the row ranges fill the device
// about four workgroups deep where the tile pairs alone do not, none shorter than IBS_SPLIT_ROWS rows
int ibs_pairs_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, hpgv_ibs_counts *d_counts,
                     hipStream_t st) {
    hpgv::IbsArgs A;
    A.gt = d_gt; A.pitch = pitch; A.n_variants = n_variants; A.n_cols = n_cols; A.skip = d_skip; A.counts = reinterpret_cast<int *>(d_counts);
    const long long tiles = ((long long)n_cols + hpgv::IBS_T - 1) / hpgv::IBS_T;
    A.pairs = tiles * (tiles + 1) / 2;
    const long long want = (4ll * ctx->n_cus + A.pairs - 1) / A.pairs, room = ((long long)n_variants + hpgv::IBS_SPLIT_ROWS - 1) / hpgv::IBS_SPLIT_ROWS;
    const long long splits = std::max(1ll, std::min(want, room));
    A.rows_per_split = (int)((((long long)n_variants + splits - 1) / splits + 63) / 64 * 64);
    A.splits = (int)(((long long)n_variants + A.rows_per_split - 1) / A.rows_per_split);
    A.items = (unsigned long long)A.pairs * (unsigned long long)A.splits;
    const unsigned long long per_xcd = (A.items + 7) / 8;
    if (per_xcd * 8 > 0x7FFFFFFFull) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d columns: %lld tile pairs exceed the grid", n_cols, A.pairs);
    A.per_xcd = (unsigned)per_xcd;
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] { hipLaunchKernelGGL(hpgv::k_ibs_pairs, dim3((unsigned)(per_xcd * 8)), dim3(256), 0, st, A); });
}

// the back half of hpgv_ibs and hpgv_ibs_text: cols_front's matrix and class counts, the pair counts added into the caller's device
// buffer, the class counts to the caller
int ibs_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, int32_t *class4, hpgv_ibs_counts *d_counts) {
    const int nv = S.n, ns = ctx->stats.n_samples;
    if (nv > 0) {
        ColsFront F;
        if (const int rc = cols_front(ctx, s, S, skip, x_too, false, &F)) return rc;
        if (ns >= 2)
            if (const int rc = ibs_pairs_launch(ctx, F.d_gt, F.pitch, nv, ns, F.d_skip, d_counts, s->stream)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(class4, F.d_class4, (size_t)nv * 16, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

int ibs_host_check(hpgv_ctx *ctx, const char *what, const hpgv_ibs_counts *d_counts) {
    if (is_group(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%s on a group context: the counts of a run lie on one device", what);
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if ((uintptr_t)d_counts & 15) return fail(ctx, HPGV_ERR_INVALID, "d_counts must be 16-byte aligned");
    if (ctx->stats.n_samples >= 2 && !d_counts) return fail(ctx, HPGV_ERR_INVALID, "d_counts is NULL");
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_ibs_pairs_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip,
                       hpgv_ibs_counts *d_counts, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = ibs_matrix_check(ctx, d_gt, pitch, n_variants, n_cols)) return rc;
    if ((uintptr_t)d_counts & 15) return fail(ctx, HPGV_ERR_INVALID, "d_counts must be 16-byte aligned");
    if (n_variants == 0 || n_cols < 2) return HPGV_OK;
    if (!d_gt || !d_counts) return fail(ctx, HPGV_ERR_INVALID, "bad ibs_pairs arguments");
    DeviceGuard g(ctx->device);
    return ibs_pairs_launch(ctx, d_gt, pitch, n_variants, n_cols, d_skip, d_counts, (hipStream_t)stream);
}

int hpgv_ibs_class_counts_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip,
                              int32_t *d_class4, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = ibs_matrix_check(ctx, d_gt, pitch, n_variants, n_cols)) return rc;
    if ((uintptr_t)d_class4 & 15) return fail(ctx, HPGV_ERR_INVALID, "d_class4 must be 16-byte aligned");
    if (n_variants == 0) return HPGV_OK;
    if (!d_gt || !d_class4) return fail(ctx, HPGV_ERR_INVALID, "bad ibs_class_counts arguments");
    DeviceGuard g(ctx->device);
    return ibs_class_launch(ctx, d_gt, pitch, n_variants, n_cols, d_skip, d_class4, (hipStream_t)stream);
}

int hpgv_ibs_select_dev(hpgv_ctx *ctx, const hpgv_ibs_counts *d_counts, int n_cols, const double E[5], double min_pi_hat, hpgv_ibs_pair *d_pairs,
                        uint64_t cap, uint64_t *d_n, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_cols < 0 || !E || !d_n || (cap > 0 && !d_pairs) || (n_cols >= 2 && !d_counts)) return fail(ctx, HPGV_ERR_INVALID, "bad ibs_select arguments");
    if (min_pi_hat != min_pi_hat) return fail(ctx, HPGV_ERR_INVALID, "min_pi_hat is NaN");
    if (((uintptr_t)d_counts & 15) || ((uintptr_t)d_pairs & 15) || ((uintptr_t)d_n & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_counts and d_pairs must be 16-byte aligned, d_n 8-byte aligned");
    const long long bpr = ((long long)n_cols + 255) / 256, wgs = bpr * n_cols;
    if (wgs > 0x7FFFFFFFll) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d columns: the matrix exceeds the grid", n_cols);
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(ctx, hipMemsetAsync(d_n, 0, sizeof(uint64_t), st));
    if (n_cols < 2) return HPGV_OK;
    hpgv::IbsE e;
    for (int k = 0; k < 5; ++k) e.e[k] = E[k];
    hipLaunchKernelGGL(hpgv::k_ibs_select, dim3((unsigned)wgs), dim3(256), 0, st, reinterpret_cast<const int4 *>(d_counts), n_cols, (int)bpr, e, min_pi_hat,
                       reinterpret_cast<uint4 *>(d_pairs), (unsigned long long)cap, (unsigned long long *)d_n);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_ibs(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *skip, int32_t *class4, hpgv_ibs_counts *d_counts) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = ibs_host_check(ctx, "hpgv_ibs", d_counts)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !class4))) return fail(ctx, HPGV_ERR_INVALID, "bad ibs arguments");
    if (pitch < (size_t)ctx->stats.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->stats.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, gt, pitch, n_variants, nullptr, &S))) return rc;
    return ibs_finish(ctx, s, S, skip, false, class4, d_counts);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_ibs_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off,
                  int32_t *status, int32_t *class4, hpgv_ibs_counts *d_counts) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = ibs_host_check(ctx, "hpgv_ibs_text", d_counts)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !class4)) return fail(ctx, HPGV_ERR_INVALID, "bad ibs_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    // the lines hpgv_assoc_text's callers drop are skipped rows, and so are the lines the tokenizer flagged as chromosome X; no
    // final layout: ibs_finish reads the tokenizer's matrix in place
    if ((rc = text_front_skip(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S, false))) return rc;
    // more lines than max_lines: NOTHING is added -- the caller calls again with room, and the counts must not hold a part twice
    if (*n_lines > max_lines) return HPGV_OK;
    return ibs_finish(ctx, s, S, K.bytes(), true, class4, d_counts);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only helpers: no GPU call, usable without a device ------------------------------------------------------------ */

int hpgv_ibs_terms(int32_t n0, int32_t n1, int32_t n2, double t[5]) { return hpgv::ibs_terms_value(n0, n1, n2, t); }

void hpgv_ibs_genome(const hpgv_ibs_counts *c, const double E[5], double out[5]) { hpgv::ibs_genome_value(c->n, c->ibs0, c->ibs1, c->ibs2, E, out); }

}  // extern "C"
