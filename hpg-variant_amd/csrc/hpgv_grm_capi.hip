// hpgv_grm_capi.hip -- C ABI of the genetic relationship matrix (include/hpgv.h "GRM"): the device-resident launches of k_grm_table
// and k_grm_pairs, the synchronous entry points on a host batch and on a text -- staged as hpgv_ibs / hpgv_ibs_text are, their
// back half shared with them (cols_back, hpgv_cols_capi.hip) -- and the host-only helpers: a row's table, the recommended frac_bits,
// the value of a pair's sums, the row-range plan.
#include "hpgv_internal.h"
#include "hpgv_grm_kernels.h"
#include <cstddef>

namespace {

static_assert(sizeof(hpgv_grm_acc) == 16 && offsetof(hpgv_grm_acc, n) == 8, "k_grm_pairs adds to a record as two int64");

int grm_params_check(const hpgv_ctx *ctx, int frac_bits, double min_maf) {
    if (frac_bits < 0 || frac_bits > hpgv::GRM_MAX_FRAC_BITS) return fail(ctx, HPGV_ERR_INVALID, "frac_bits %d: 0 .. %d", frac_bits, hpgv::GRM_MAX_FRAC_BITS);
    if (!(min_maf >= 0.0 && min_maf <= 0.5)) return fail(ctx, HPGV_ERR_INVALID, "min_maf %g: 0 .. 0.5", min_maf);
    return HPGV_OK;
}

int grm_table_launch(hpgv_ctx *ctx, const int32_t *d_class4, int n_variants, int frac_bits, double min_maf, uint8_t *d_skip, uint8_t *d_tab, int32_t *d_n_used,
                     hipStream_t st) {
    if (d_n_used) HIPCHK(ctx, hipMemsetAsync(d_n_used, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(hpgv::k_grm_table, dim3((unsigned)(((long long)n_variants + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const int4 *>(d_class4), n_variants,
                       frac_bits, min_maf, d_skip, reinterpret_cast<uint2 *>(d_tab), d_n_used);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

// the launch of k_grm_pairs (the arguments checked, the device current, rows and columns to do) in the row ranges of grm_plan_rows
int grm_pairs_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, const uint8_t *d_tab, hpgv_grm_acc *d_acc,
                     hipStream_t st) {
    hpgv::GrmArgs A;
    A.tab = reinterpret_cast<const uint2 *>(d_tab);
    A.acc = reinterpret_cast<long long *>(d_acc);
    if (const int rc = cols_grid_fill(ctx, d_gt, pitch, n_variants, n_cols, d_skip, hpgv::cols_tile_pairs(n_cols), hpgv::grm_plan_rows(n_variants, n_cols, ctx->n_cus),
                                      "tile pairs", &A.G))
        return rc;
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] { hipLaunchKernelGGL(hpgv::k_grm_pairs, dim3(A.G.per_xcd * 8), dim3(256), 0, st, A); });
}

// the back half of hpgv_grm and hpgv_grm_text: the rows' tables (which mark the unused rows skipped), the pair sums added into the
// caller's device buffer, from 1 sample on
int grm_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, int frac_bits, double min_maf, int32_t *class4, hpgv_grm_acc *d_acc) {
    const int nv = S.n, ns = ctx->stats.n_samples;
    return cols_back(ctx, s, S, skip, x_too, true, class4, [&](const ColsFront &F) {
        if (ns < 1) return (int)HPGV_OK;
        HIPCHK(ctx, s->dbl.reserve_slack((size_t)nv * 8 + 16));
        if (const int rc = grm_table_launch(ctx, F.d_class4, nv, frac_bits, min_maf, F.d_skip, s->dbl.as<uint8_t>(), nullptr, s->stream)) return rc;
        return grm_pairs_launch(ctx, F.d_gt, F.pitch, nv, ns, F.d_skip, s->dbl.as<uint8_t>(), d_acc, s->stream);
    });
}

int grm_host_check(hpgv_ctx *ctx, const char *what, int frac_bits, double min_maf, const hpgv_grm_acc *d_acc) {
    if (is_group(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%s on a group context: the sums of a run lie on one device", what);
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (const int rc = grm_params_check(ctx, frac_bits, min_maf)) return rc;
    if ((uintptr_t)d_acc & 15) return fail(ctx, HPGV_ERR_INVALID, "d_acc must be 16-byte aligned");
    if (ctx->stats.n_samples >= 1 && !d_acc) return fail(ctx, HPGV_ERR_INVALID, "d_acc is NULL");
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_grm_table_dev(hpgv_ctx *ctx, const int32_t *d_class4, int n_variants, int frac_bits, double min_maf, uint8_t *d_skip, uint8_t *d_tab, int32_t *d_n_used,
                       void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0) return fail(ctx, HPGV_ERR_INVALID, "bad grm_table arguments: %d rows", n_variants);
    if (const int rc = grm_params_check(ctx, frac_bits, min_maf)) return rc;
    if (((uintptr_t)d_class4 & 15) || ((uintptr_t)d_tab & 7) || ((uintptr_t)d_n_used & 3))
        return fail(ctx, HPGV_ERR_INVALID, "d_class4 must be 16-byte aligned, d_tab 8-byte aligned, d_n_used 4-byte aligned");
    DeviceGuard g(ctx->device);
    if (n_variants == 0) {
        if (d_n_used) HIPCHK(ctx, hipMemsetAsync(d_n_used, 0, sizeof(int32_t), (hipStream_t)stream));
        return HPGV_OK;
    }
    if (!d_class4 || !d_skip || !d_tab) return fail(ctx, HPGV_ERR_INVALID, "bad grm_table arguments: d_class4, d_skip and d_tab are required");
    return grm_table_launch(ctx, d_class4, n_variants, frac_bits, min_maf, d_skip, d_tab, d_n_used, (hipStream_t)stream);
}

int hpgv_grm_pairs_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, const uint8_t *d_tab,
                       hpgv_grm_acc *d_acc, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = cols_matrix_check(ctx, d_gt, pitch, n_variants, n_cols)) return rc;
    if (((uintptr_t)d_acc & 15) || ((uintptr_t)d_tab & 7)) return fail(ctx, HPGV_ERR_INVALID, "d_acc must be 16-byte aligned, d_tab 8-byte aligned");
    if (n_variants == 0 || n_cols < 1) return HPGV_OK;
    if (!d_gt || !d_tab || !d_acc) return fail(ctx, HPGV_ERR_INVALID, "bad grm_pairs arguments");
    DeviceGuard g(ctx->device);
    return grm_pairs_launch(ctx, d_gt, pitch, n_variants, n_cols, d_skip, d_tab, d_acc, (hipStream_t)stream);
}

int hpgv_grm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *skip, int frac_bits, double min_maf, int32_t *class4,
             hpgv_grm_acc *d_acc) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = grm_host_check(ctx, "hpgv_grm", frac_bits, min_maf, d_acc)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !class4))) return fail(ctx, HPGV_ERR_INVALID, "bad grm arguments");
    if (pitch < (size_t)ctx->stats.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->stats.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, gt, pitch, n_variants, nullptr, &S))) return rc;
    return grm_finish(ctx, s, S, skip, false, frac_bits, min_maf, class4, d_acc);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_grm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off, int32_t *status,
                  int frac_bits, double min_maf, int32_t *class4, hpgv_grm_acc *d_acc) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = grm_host_check(ctx, "hpgv_grm_text", frac_bits, min_maf, d_acc)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !class4)) return fail(ctx, HPGV_ERR_INVALID, "bad grm_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    // as hpgv_ibs_text: dropped lines and chromosome-X lines are skipped rows, the tokenizer's matrix is read in place
    if ((rc = text_front_skip(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S, false))) return rc;
    // more lines than max_lines: NOTHING is added -- the caller calls again with room, and the sums must not hold a part twice
    if (*n_lines > max_lines) return HPGV_OK;
    return grm_finish(ctx, s, S, K.bytes(), true, frac_bits, min_maf, class4, d_acc);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only helpers: no GPU call, usable without a device ------------------------------------------------------------ */

int hpgv_grm_table(int32_t n0, int32_t n1, int32_t n2, int frac_bits, double min_maf, int8_t hi[4], int8_t lo[4]) {
    return hpgv::grm_table_value(n0, n1, n2, frac_bits, min_maf, hi, lo);
}

int hpgv_grm_frac_bits(double min_maf) {
    if (!(min_maf > 0.0 && min_maf <= 0.5)) return -1;
    const double z = sqrt(2.0 * (1.0 - min_maf) / min_maf);
    for (int s = hpgv::GRM_MAX_FRAC_BITS; s >= 0; --s)
        if (z * (double)(1 << s) <= (double)hpgv::GRM_MAX_Q) return s;
    return -1;
}

double hpgv_grm_value(const hpgv_grm_acc *a, int frac_bits) { return hpgv::grm_value(a->sq, a->n, frac_bits); }

int hpgv_grm_plan_rows(int n_variants, int n_cols, int n_cus) { return hpgv::grm_plan_rows(n_variants, n_cols, n_cus); }

}  // extern "C"
