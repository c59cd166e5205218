// hpgv_ibs_capi.hip -- C ABI of the sample-relatedness counts (include/hpgv.h "IBS"): the device-resident launches of k_ibs_pairs,
// the class counts and k_ibs_select, the synchronous entry points on a host batch and on a text -- staged like every tool's, by
// stage_chain and text_front_skip (hpgv_internal.h), through the STATS layout: every sample, in VCF order; their back half is
// cols_back's (hpgv_cols_capi.hip) -- and the host-only helpers: the terms of a row's class counts, the genome values of a pair's
// counts, the row-range plan.
#include "hpgv_internal.h"
#include "hpgv_ibs_kernels.h"
#include <cstddef>

namespace {

static_assert(sizeof(hpgv_ibs_counts) == 16, "k_ibs_pairs adds to a record as four int32, k_ibs_select loads it as one int4");
static_assert(sizeof(hpgv_ibs_pair) == 32 && offsetof(hpgv_ibs_pair, j) == 4 && offsetof(hpgv_ibs_pair, c) == 8 && offsetof(hpgv_ibs_pair, pi_hat) == 24,
              "k_ibs_select stores a record as two uint4");

// the launch of k_ibs_pairs (the arguments checked, the device current, rows and pairs to do) in the row ranges of ibs_plan_rows
int ibs_pairs_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, hpgv_ibs_counts *d_counts,
                     hipStream_t st) {
    hpgv::IbsArgs A;
    A.counts = reinterpret_cast<int *>(d_counts);
    if (const int rc = cols_grid_fill(ctx, d_gt, pitch, n_variants, n_cols, d_skip, hpgv::cols_tile_pairs(n_cols), hpgv::ibs_plan_rows(n_variants, n_cols, ctx->n_cus),
                                      "tile pairs", &A.G))
        return rc;
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] { hipLaunchKernelGGL(hpgv::k_ibs_pairs, dim3(A.G.per_xcd * 8), dim3(256), 0, st, A); });
}

// the back half of hpgv_ibs and hpgv_ibs_text: the pair counts added into the caller's device buffer, from 2 samples on
int ibs_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, int32_t *class4, hpgv_ibs_counts *d_counts) {
    const int ns = ctx->stats.n_samples;
    return cols_back(ctx, s, S, skip, x_too, false, class4, [&](const ColsFront &F) {
        return ns >= 2 ? ibs_pairs_launch(ctx, F.d_gt, F.pitch, S.n, ns, F.d_skip, d_counts, s->stream) : HPGV_OK;
    });
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
    if (const int rc = cols_matrix_check(ctx, d_gt, pitch, n_variants, n_cols)) return rc;
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
    if (const int rc = cols_matrix_check(ctx, d_gt, pitch, n_variants, n_cols)) return rc;
    if ((uintptr_t)d_class4 & 15) return fail(ctx, HPGV_ERR_INVALID, "d_class4 must be 16-byte aligned");
    if (n_variants == 0) return HPGV_OK;
    if (!d_gt || !d_class4) return fail(ctx, HPGV_ERR_INVALID, "bad ibs_class_counts arguments");
    DeviceGuard g(ctx->device);
    return cols_class_launch(ctx, d_gt, pitch, n_variants, n_cols, d_skip, d_class4, (hipStream_t)stream);
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

int hpgv_ibs_plan_rows(int n_variants, int n_cols, int n_cus) { return hpgv::ibs_plan_rows(n_variants, n_cols, n_cus); }

}  // extern "C"
