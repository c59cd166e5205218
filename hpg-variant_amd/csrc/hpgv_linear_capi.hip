// hpgv_linear_capi.hip -- C ABI of the linear regression (include/hpgv.h "Linear regression"): the phenotype of a context and the
// model's device image, the device-resident launch of k_linear, the synchronous entry points on a host batch and on a text --
// built as hpgv_assoc_logistic's are: arguments, a slot, stage_chain / text_front, then the regressions' back half (regression_finish, hpgv_internal.h) -- the host-only fit
// and the t tail.
#include "hpgv_internal.h"
#include "hpgv_linear_kernels.h"

namespace {

static_assert(sizeof(hpgv_linear_result) == 48 && offsetof(hpgv_linear_result, n_obs) == 32, "the record of include/hpgv.h");

constexpr int Q = hpgv::LINEAR_Q;

// The model of n_pos positions, col(pos) the sample behind a position or -1 for a pad: feat[pos * Q + f] the centred features
// [1, c_1 - m_1 .. c_C - m_C, y - m_y] (zeros under pads and in unused columns), G = sum f f^T and the means, the sums over the
// positions in ascending order with one fma per term.  The device image and the host fit both come from here.
template <class Col>
void linear_model(size_t n_pos, Col col, const double *y, const double *cov, int C, double *feat, double *G, double *mean) {
    const int q = C + 2;
    for (int f = 0; f < Q; ++f) mean[f] = 0.0;
    for (int f = 0; f < Q * Q; ++f) G[f] = 0.0;
    size_t n = 0;
    for (size_t pos = 0; pos < n_pos; ++pos) {
        const long j = col(pos);
        if (j < 0) continue;
        ++n;
        for (int k = 0; k < C; ++k) mean[1 + k] += cov[(size_t)j * (size_t)C + (size_t)k];
        mean[q - 1] += y[j];
    }
    if (n) for (int f = 1; f < q; ++f) mean[f] /= (double)n;
    for (size_t pos = 0; pos < n_pos; ++pos) {
        double *f = feat + pos * Q;
        for (int k = 0; k < Q; ++k) f[k] = 0.0;
        const long j = col(pos);
        if (j < 0) continue;
        f[0] = 1.0;
        for (int k = 0; k < C; ++k) f[1 + k] = cov[(size_t)j * (size_t)C + (size_t)k] - mean[1 + k];
        f[q - 1] = y[j] - mean[q - 1];
        for (int a = 0; a < q; ++a)
            for (int b = a; b < q; ++b) G[a * Q + b] = fma(f[a], f[b], G[a * Q + b]);
    }
    for (int a = 0; a < q; ++a)
        for (int b = 0; b < a; ++b) G[a * Q + b] = G[b * Q + a];
}

size_t image_positions(const hpgv_ctx *ctx) { return round_up(ctx->assoc.pitch, (size_t)64); }

int linear_state_check(const hpgv_ctx *ctx) {
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (!ctx->has_pheno) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_phenotype has not been called");
    return HPGV_OK;
}

// the launch on `st`: one workgroup per 16 rows
int linear_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, hpgv_linear_result *d_out, double *d_coef, hipStream_t st) {
    if (n_variants == 0) return HPGV_OK;
    if (ctx->assoc.pitch % 16) return fail(ctx, HPGV_ERR_UNSUPPORTED, "the linear regression needs a row pitch that is a multiple of 16");
    hpgv::LinArgs A;
    A.gt = d_gt; A.pitch = ctx->assoc.pitch; A.n_variants = n_variants;
    A.nA = ctx->nA; A.segA = ctx->chunksA * 16; A.nU = ctx->nU;
    A.n_covar = ctx->n_covar;
    A.feat = ctx->d_lin.as<double>(); A.G = A.feat + image_positions(ctx) * Q; A.mean = A.G + Q * Q;
    A.out = d_out; A.coef = d_coef;
    const dim3 grid((unsigned)((n_variants + hpgv::LINEAR_ROWS - 1) / hpgv::LINEAR_ROWS)), block(256);
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] { hipLaunchKernelGGL(hpgv::k_linear, grid, block, 0, st, A); });
}

}  // namespace

// the image of the context's phenotype and covariates, or nothing without a phenotype
int linear_image_rebuild(hpgv_ctx *ctx) {
    if (!ctx->has_pheno) return HPGV_OK;
    const Layout &L = ctx->assoc;
    const int C = ctx->n_covar;
    const size_t n_pos = image_positions(ctx);
    std::vector<double> img(n_pos * Q + Q * Q + Q);
    linear_model(n_pos, [&](size_t pos) { return pos < L.pitch ? (long)L.col_of_pos[pos] : -1L; }, ctx->lin_y.data(), ctx->lin_cov.data(), C,
                 img.data(), img.data() + n_pos * Q, img.data() + n_pos * Q + Q * Q);
    DeviceGuard g(ctx->device);
    const hipError_t e = ctx->d_lin.reserve(img.size() * sizeof(double));
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); ctx->has_pheno = false; return fail(ctx, HPGV_ERR_NOMEM, "the linear model (%zu bytes) does not fit the device", img.size() * sizeof(double)); }
    HIPCHK(ctx, e);
    HIPCHK(ctx, hipMemcpy(ctx->d_lin.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    return HPGV_OK;
}

extern "C" {

int hpgv_set_phenotype(hpgv_ctx *ctx, const double *y, int n_samples) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_phenotype(m_, y, n_samples))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (!y) { ctx->has_pheno = false; ctx->lin_y.clear(); return HPGV_OK; }
    const Layout &L = ctx->assoc;
    if (n_samples != L.n_samples) return fail(ctx, HPGV_ERR_INVALID, "a phenotype for %d samples: the cohort has %d columns", n_samples, L.n_samples);
    for (size_t pos = 0; pos < L.pitch; ++pos) {
        const int32_t j = L.col_of_pos[pos];
        if (j >= 0 && !std::isfinite(y[j])) return fail(ctx, HPGV_ERR_INVALID, "the phenotype of column %d is not finite", (int)j);
    }
    ctx->lin_y.assign(y, y + n_samples);
    for (int j = 0; j < n_samples; ++j) if (!std::isfinite(ctx->lin_y[(size_t)j])) ctx->lin_y[(size_t)j] = 0.0;      // (OTHER columns: never read)
    ctx->has_pheno = true;
    return linear_image_rebuild(ctx);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_linear_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, hpgv_linear_result *d_out, double *d_coef, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = linear_state_check(ctx)) return rc;
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_out))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_linear arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_coef & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_out must be 16-byte aligned, d_coef 8-byte aligned");
    DeviceGuard g(ctx->device);
    return linear_launch(ctx, d_gt, n_variants, d_out, d_coef, (hipStream_t)stream);
}

int hpgv_assoc_linear(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, hpgv_linear_result *out, double *coef) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_linear(m_, gt, pitch, n_variants, out, coef))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = linear_state_check(ctx)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !out))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_linear arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    return regression_finish(ctx, s, S, out, coef, linear_launch);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_linear_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines, uint64_t *line_off,
                           uint32_t *field_off, int32_t *status, hpgv_linear_result *out, double *coef) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_linear_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, out, coef))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = linear_state_check(ctx)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !out)) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_linear_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S))) return rc;
    return regression_finish(ctx, s, S, out, coef, linear_launch);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only: no GPU call, usable without a device ------------------------------------------------------------- */

int hpgv_linear_fit(const uint8_t *cls, const double *y, const double *cov, int n, int n_covar, hpgv_linear_result *out, double *coef) {
    if (n < 0 || n_covar < 0 || n_covar > HPGV_LOGISTIC_MAX_COVAR || !out || (n > 0 && (!cls || !y || (n_covar > 0 && !cov)))) return HPGV_ERR_INVALID;
    for (int s = 0; s < n; ++s) {
        if (!std::isfinite(y[s])) return HPGV_ERR_INVALID;
        for (int k = 0; k < n_covar; ++k) if (!std::isfinite(cov[(size_t)s * (size_t)n_covar + (size_t)k])) return HPGV_ERR_INVALID;
    }
    try {
        constexpr int LD = hpgv::LOGIT_LD, MAXP = hpgv::LOGIT_MAXP;
        const int q = n_covar + 2;
        std::vector<double> feat((size_t)n * Q + 1);
        double G[Q * Q], mean[Q], S[Q * Q], h[Q] = {0.0}, A[MAXP * LD], X[MAXP * LD], V[MAXP * LD], D[MAXP];
        linear_model((size_t)n, [](size_t pos) { return (long)pos; }, y, cov, n_covar, feat.data(), G, mean);
        int n1 = 0, n2 = 0, n_obs = 0;
        for (int s = 0; s < n; ++s) {
            if (cls[s] > 2) continue;
            ++n_obs; n1 += cls[s] == 1; n2 += cls[s] == 2;
            for (int f = 0; f < q; ++f) h[f] = fma((double)cls[s], feat[(size_t)s * Q + f], h[f]);
        }
        const bool direct = n - n_obs > n_obs;
        for (int f = 0; f < Q * Q; ++f) S[f] = direct ? 0.0 : G[f];
        for (int s = 0; s < n; ++s) {
            if ((cls[s] > 2) == direct) continue;
            const double *f = feat.data() + (size_t)s * Q, sign = direct ? 1.0 : -1.0;
            for (int a = 0; a < q; ++a)
                for (int b = a; b < q; ++b) S[a * Q + b] = fma(sign * f[a], f[b], S[a * Q + b]);
        }
        for (int a = 0; a < q; ++a)
            for (int b = 0; b < a; ++b) S[a * Q + b] = S[b * Q + a];
        hpgv::linear_record(n_covar, S, h, n1, n2, n_obs, mean, A, X, V, D, 0, 1, [] {}, out, coef);
    } catch (const std::bad_alloc &) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

double hpgv_linear_t_p(double t, int df) { return hpgv::linear_t_p(t, df); }

}  // extern "C"
