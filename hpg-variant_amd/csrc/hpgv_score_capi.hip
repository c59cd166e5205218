// hpgv_score_capi.hip -- C ABI of allele scoring (include/hpgv.h "Score"): the device-resident launches of k_score_table and
// k_score_cols, the synchronous entry points on a host batch and on a text -- staged as hpgv_grm / hpgv_grm_text are, their back half
// shared with them (cols_back, hpgv_cols_capi.hip); the text form asks the caller for the rows' weights once the line heads are
// back -- and the host-only helpers: a row's table, the recommended frac_bits, the value of a sum, the row-range plan.
#include "hpgv_internal.h"
#include "hpgv_score_kernels.h"
#include <climits>
#include <cmath>
#include <cstddef>

namespace {

static_assert(HPGV_SCORE_MAX == hpgv::SCORE_MAX, "include/hpgv.h and the kernels header");

int score_params_check(const hpgv_ctx *ctx, int n_scores, const int *s) {
    if (n_scores < 1 || n_scores > hpgv::SCORE_MAX) return fail(ctx, HPGV_ERR_INVALID, "n_scores %d: 1 .. %d", n_scores, hpgv::SCORE_MAX);
    if (!s) return fail(ctx, HPGV_ERR_INVALID, "frac_bits is NULL");
    for (int k = 0; k < n_scores; ++k)
        if (s[k] < -hpgv::SCORE_MAX_FRAC_BITS || s[k] > hpgv::SCORE_MAX_FRAC_BITS)
            return fail(ctx, HPGV_ERR_INVALID, "frac_bits[%d] = %d: -%d .. %d", k, s[k], hpgv::SCORE_MAX_FRAC_BITS, hpgv::SCORE_MAX_FRAC_BITS);
    return HPGV_OK;
}

int score_pitch_check(const hpgv_ctx *ctx, int n_variants, size_t tab_pitch) {
    if (n_variants < 0) return fail(ctx, HPGV_ERR_INVALID, "bad score arguments: %d rows", n_variants);
    if ((tab_pitch & 63) || tab_pitch < (size_t)n_variants) return fail(ctx, HPGV_ERR_INVALID, "tab_pitch %zu: a multiple of 64, at least %d rows", tab_pitch, n_variants);
    return HPGV_OK;
}

int score_table_launch(hpgv_ctx *ctx, const int32_t *d_class4, int n_variants, const double *d_w, const uint8_t *d_flags, int n_scores, const int *s, int impute,
                       uint8_t *d_skip, int8_t *d_tab, size_t tab_pitch, int64_t *d_const, hipStream_t st) {
    hpgv::ScoreS S{};
    for (int k = 0; k < n_scores; ++k) S.s[k] = s[k];
    hipLaunchKernelGGL(hpgv::k_score_table, dim3((unsigned)((tab_pitch + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const int4 *>(d_class4), n_variants, d_w,
                       d_flags, n_scores, S, impute ? 1 : 0, d_skip, d_tab, tab_pitch, reinterpret_cast<long long *>(d_const));
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

// the launch of k_score_cols (the arguments checked, the device current, rows and columns to do) in the row ranges of score_plan_rows
int score_cols_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, const int8_t *d_tab, size_t tab_pitch,
                      int n_scores, int64_t *d_acc, size_t acc_pitch, hipStream_t st) {
    hpgv::ScoreArgs A;
    A.tab = d_tab; A.tab_pitch = tab_pitch; A.n_scores = n_scores;
    A.acc = reinterpret_cast<long long *>(d_acc); A.acc_pitch = acc_pitch;
    if (const int rc = cols_grid_fill(ctx, d_gt, pitch, n_variants, n_cols, d_skip, hpgv::cols_tiles(n_cols), hpgv::score_plan_rows(n_variants, n_cols, n_scores, ctx->n_cus),
                                      "column tiles", &A.G))
        return rc;
    const dim3 grid(A.G.per_xcd * 8), block(256);
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
        switch ((n_scores + 3) / 4) {
        case 1: hipLaunchKernelGGL(hpgv::k_score_cols<1>, grid, block, 0, st, A); break;
        case 2: hipLaunchKernelGGL(hpgv::k_score_cols<2>, grid, block, 0, st, A); break;
        case 3: hipLaunchKernelGGL(hpgv::k_score_cols<3>, grid, block, 0, st, A); break;
        case 4: hipLaunchKernelGGL(hpgv::k_score_cols<4>, grid, block, 0, st, A); break;
        case 5: hipLaunchKernelGGL(hpgv::k_score_cols<5>, grid, block, 0, st, A); break;
        case 6: hipLaunchKernelGGL(hpgv::k_score_cols<6>, grid, block, 0, st, A); break;
        case 7: hipLaunchKernelGGL(hpgv::k_score_cols<7>, grid, block, 0, st, A); break;
        default: hipLaunchKernelGGL(hpgv::k_score_cols<8>, grid, block, 0, st, A); break;
        }
    });
}

// where the per-call arrays of a host entry lie in the slot's `dbl`: the weights, the limb planes, the flag bytes
struct ScoreRoom {
    double *d_w;
    int8_t *d_tab;
    uint8_t *d_flags;
    size_t tab_pitch;
};

int score_room(hpgv_ctx *ctx, Slot *s, int nv, int n_scores, ScoreRoom *R) {
    const size_t n = (size_t)nv, tab_pitch = (n + 63) / 64 * 64;
    const size_t w_bytes = (n * (size_t)n_scores * sizeof(double) + 63) / 64 * 64, tab_bytes = tab_pitch * 8 * (size_t)n_scores;
    HIPCHK(ctx, s->dbl.reserve_slack(w_bytes + tab_bytes + n + 64));
    R->d_w = s->dbl.as<double>();
    R->d_tab = s->dbl.as<int8_t>() + w_bytes;
    R->d_flags = s->dbl.as<uint8_t>() + w_bytes + tab_bytes;
    R->tab_pitch = tab_pitch;
    return HPGV_OK;
}

// the back half of hpgv_score and hpgv_score_text (skip: bit 0 of the flags, and what the text form skips): the rows' tables (which
// mark the unused rows skipped), the sums added into the caller's device buffers, from 1 sample on
int score_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, const double *w, const uint8_t *flags, int n_scores, const int *frac_bits,
                 int impute, int32_t *class4, int64_t *d_acc, size_t acc_pitch, int64_t *d_const) {
    const int nv = S.n, ns = ctx->stats.n_samples;
    return cols_back(ctx, s, S, skip, x_too, true, class4, [&](const ColsFront &F) {
        ScoreRoom R;
        if (const int rc = score_room(ctx, s, nv, n_scores, &R)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(R.d_w, w, (size_t)nv * (size_t)n_scores * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(R.d_flags, flags, (size_t)nv, hipMemcpyHostToDevice, s->stream));
        if (const int rc = score_table_launch(ctx, F.d_class4, nv, R.d_w, R.d_flags, n_scores, frac_bits, impute, F.d_skip, R.d_tab, R.tab_pitch, d_const, s->stream))
            return rc;
        return ns >= 1 ? score_cols_launch(ctx, F.d_gt, F.pitch, nv, ns, F.d_skip, R.d_tab, R.tab_pitch, n_scores, d_acc, acc_pitch, s->stream) : (int)HPGV_OK;
    });
}

int score_host_check(hpgv_ctx *ctx, const char *what, int n_scores, const int *frac_bits, const int64_t *d_acc, size_t acc_pitch, const int64_t *d_const) {
    if (is_group(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%s on a group context: the sums of a run lie on one device", what);
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (const int rc = score_params_check(ctx, n_scores, frac_bits)) return rc;
    if (((uintptr_t)d_acc & 7) || ((uintptr_t)d_const & 7)) return fail(ctx, HPGV_ERR_INVALID, "d_acc and d_const must be 8-byte aligned");
    if (!d_const || (ctx->stats.n_samples >= 1 && !d_acc)) return fail(ctx, HPGV_ERR_INVALID, "d_acc or d_const is NULL");
    if (acc_pitch < (size_t)ctx->stats.n_samples) return fail(ctx, HPGV_ERR_INVALID, "acc_pitch %zu < n_samples %d", acc_pitch, ctx->stats.n_samples);
    return HPGV_OK;
}

// every weight finite: checked on the host before anything is launched
int score_weights_check(const hpgv_ctx *ctx, const double *w, size_t n_rows, int n_scores) {
    for (size_t i = 0; i < n_rows * (size_t)n_scores; ++i)
        if (!std::isfinite(w[i])) return fail(ctx, HPGV_ERR_INVALID, "weight %zu of row %zu is not finite", i % (size_t)n_scores, i / (size_t)n_scores);
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_score_table_dev(hpgv_ctx *ctx, const int32_t *d_class4, int n_variants, const double *d_w, const uint8_t *d_flags, int n_scores, const int *frac_bits,
                         int impute, uint8_t *d_skip, int8_t *d_tab, size_t tab_pitch, int64_t *d_const, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = score_params_check(ctx, n_scores, frac_bits)) return rc;
    if (const int rc = score_pitch_check(ctx, n_variants, tab_pitch)) return rc;
    if (((uintptr_t)d_class4 & 15) || ((uintptr_t)d_tab & 15) || ((uintptr_t)d_w & 7) || ((uintptr_t)d_const & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_class4 and d_tab must be 16-byte aligned, d_w and d_const 8-byte aligned");
    if (tab_pitch == 0) return HPGV_OK;
    if (!d_tab || !d_const || (n_variants > 0 && (!d_class4 || !d_w || !d_flags || !d_skip)))
        return fail(ctx, HPGV_ERR_INVALID, "bad score_table arguments: d_class4, d_w, d_flags, d_skip, d_tab and d_const are required");
    DeviceGuard g(ctx->device);
    return score_table_launch(ctx, d_class4, n_variants, d_w, d_flags, n_scores, frac_bits, impute, d_skip, d_tab, tab_pitch, d_const, (hipStream_t)stream);
}

int hpgv_score_cols_dev(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, const int8_t *d_tab, size_t tab_pitch,
                        int n_scores, int64_t *d_acc, size_t acc_pitch, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = cols_matrix_check(ctx, d_gt, pitch, n_variants, n_cols)) return rc;
    if (n_scores < 1 || n_scores > hpgv::SCORE_MAX) return fail(ctx, HPGV_ERR_INVALID, "n_scores %d: 1 .. %d", n_scores, hpgv::SCORE_MAX);
    if (const int rc = score_pitch_check(ctx, n_variants, tab_pitch)) return rc;
    if (((uintptr_t)d_tab & 15) || ((uintptr_t)d_acc & 7)) return fail(ctx, HPGV_ERR_INVALID, "d_tab must be 16-byte aligned, d_acc 8-byte aligned");
    if (acc_pitch < (size_t)n_cols) return fail(ctx, HPGV_ERR_INVALID, "acc_pitch %zu < n_cols %d", acc_pitch, n_cols);
    if (n_variants == 0 || n_cols < 1) return HPGV_OK;
    if (!d_gt || !d_tab || !d_acc) return fail(ctx, HPGV_ERR_INVALID, "bad score_cols arguments");
    DeviceGuard g(ctx->device);
    return score_cols_launch(ctx, d_gt, pitch, n_variants, n_cols, d_skip, d_tab, tab_pitch, n_scores, d_acc, acc_pitch, (hipStream_t)stream);
}

int hpgv_score(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const double *w, const uint8_t *flags, int n_scores, const int *frac_bits, int impute,
               int32_t *class4, int64_t *d_acc, size_t acc_pitch, int64_t *d_const) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = score_host_check(ctx, "hpgv_score", n_scores, frac_bits, d_acc, acc_pitch, d_const)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !class4 || !w || !flags))) return fail(ctx, HPGV_ERR_INVALID, "bad score arguments");
    if (pitch < (size_t)ctx->stats.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->stats.n_samples);
    if (n_variants == 0) return HPGV_OK;
    if (const int rc0 = score_weights_check(ctx, w, (size_t)n_variants, n_scores)) return rc0;
    std::vector<uint8_t> skip((size_t)n_variants);
    for (int i = 0; i < n_variants; ++i) skip[(size_t)i] = flags[i] & 1;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, gt, pitch, n_variants, nullptr, &S))) return rc;
    return score_finish(ctx, s, S, skip.data(), false, w, flags, n_scores, frac_bits, impute, class4, d_acc, acc_pitch, d_const);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_score_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off, int32_t *status,
                    hpgv_score_weigh_fn weigh, void *user, int n_scores, const int *frac_bits, int impute, int32_t *class4, int64_t *d_acc, size_t acc_pitch,
                    int64_t *d_const) {
    HPGV_ABI_TRY
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = score_host_check(ctx, "hpgv_score_text", n_scores, frac_bits, d_acc, acc_pitch, d_const)) return rc0;
    if (!n_lines || !weigh || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !class4)) return fail(ctx, HPGV_ERR_INVALID, "bad score_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    // what the callback reads lies on the host whether or not the caller asked for it (all before the lease)
    TextSkip K;
    std::vector<uint64_t> own_line_off;
    std::vector<uint32_t> own_field_off;
    std::vector<int32_t> own_status;
    std::vector<double> w;
    std::vector<uint8_t> flags;
    if (!line_off) { own_line_off.assign((size_t)max_lines + 1, 0); line_off = own_line_off.data(); }
    if (!field_off) { own_field_off.assign((size_t)max_lines * 10, 0); field_off = own_field_off.data(); }
    if (!status) { own_status.assign((size_t)max_lines, 0); status = own_status.data(); }
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    // as hpgv_grm_text: dropped lines and chromosome-X lines are skipped rows, the tokenizer's matrix is read in place
    if ((rc = text_front_skip(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S, false))) return rc;
    // more lines than max_lines: NOTHING is added and the callback is not invoked -- the caller calls again with room
    if (*n_lines > max_lines) return HPGV_OK;
    const int nl = S.n;
    w.assign((size_t)nl * (size_t)n_scores, 0.0);
    flags.assign((size_t)nl, 0);
    if (nl > 0) {
        if (weigh(user, text, nl, line_off, field_off, status, w.data(), flags.data()) != 0) return fail(ctx, HPGV_ERR_INVALID, "the weigh callback refused the text");
        if ((rc = score_weights_check(ctx, w.data(), (size_t)nl, n_scores))) return rc;
        for (int i = 0; i < nl; ++i)
            if (flags[(size_t)i] & 1) K.skip[(size_t)i] = 1;
    }
    return score_finish(ctx, s, S, K.bytes(), true, w.data(), flags.data(), n_scores, frac_bits, impute, class4, d_acc, acc_pitch, d_const);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only helpers: no GPU call, usable without a device ------------------------------------------------------------ */

int hpgv_score_table(int32_t n0, int32_t n1, int32_t n2, const double *w, int n_scores, const int *frac_bits, int flags, int impute, int8_t *limbs, int64_t *c) {
    if (n_scores < 1 || n_scores > hpgv::SCORE_MAX || !w || !frac_bits || !limbs || !c) return 0;
    for (int k = 0; k < n_scores; ++k)
        if (frac_bits[k] < -hpgv::SCORE_MAX_FRAC_BITS || frac_bits[k] > hpgv::SCORE_MAX_FRAC_BITS) {
            for (int i = 0; i < n_scores; ++i) { c[i] = 0; for (int l = 0; l < 8; ++l) limbs[i * 8 + l] = 0; }
            return 0;
        }
    long long cc[hpgv::SCORE_MAX];
    const int used = hpgv::score_table_value(n0, n1, n2, w, n_scores, frac_bits, flags, impute, limbs, cc);
    for (int k = 0; k < n_scores; ++k) c[k] = cc[k];
    return used;
}

int hpgv_score_frac_bits(double max_abs_w) {
    if (!(max_abs_w >= 0.0) || std::isinf(max_abs_w)) return INT_MIN;
    if (max_abs_w == 0.0) return 0;
    int e = 0;
    (void)frexp(max_abs_w, &e);
    const int s = 28 - e;
    return s > hpgv::SCORE_MAX_FRAC_BITS ? hpgv::SCORE_MAX_FRAC_BITS : (s < -hpgv::SCORE_MAX_FRAC_BITS ? -hpgv::SCORE_MAX_FRAC_BITS : s);
}

double hpgv_score_value(int64_t sum, int64_t cnst, int frac_bits) { return hpgv::score_value(sum, cnst, frac_bits); }

int hpgv_score_plan_rows(int n_variants, int n_cols, int n_scores, int n_cus) { return hpgv::score_plan_rows(n_variants, n_cols, n_scores, n_cus); }

}  // extern "C"
