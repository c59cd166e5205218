// hpgv_logistic_capi.hip -- C ABI of the logistic regression (include/hpgv.h "Logistic regression"): the covariates of a context,
// the device-resident launch of k_logistic, the synchronous entry points on a host batch and on a text -- built as
// hpgv_assoc_model's are: arguments, a slot, stage_chain / text_front, then the regressions' back half (regression_finish, hpgv_internal.h) -- and the host-only fit.
#include "hpgv_internal.h"
#include "hpgv_logistic_kernels.h"

namespace {

static_assert(sizeof(hpgv_logistic_result) == 48 && offsetof(hpgv_logistic_result, n_obs) == 32, "the record of include/hpgv.h");

int logistic_args_check(const hpgv_ctx *ctx, int max_iter, double tol) {
    if (max_iter < 1 || max_iter > 100) return fail(ctx, HPGV_ERR_INVALID, "max_iter %d: 1 .. 100", max_iter);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ctx, HPGV_ERR_INVALID, "tol must be finite and not negative");
    return HPGV_OK;
}

// the launch on `st`: one workgroup per row, the instantiation by p = n_covar + 2
int logistic_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int max_iter, double tol, hpgv_logistic_result *d_out, double *d_coef,
                    hipStream_t st) {
    if (n_variants == 0) return HPGV_OK;
    hpgv::LogitArgs A;
    A.gt = d_gt; A.pitch = ctx->assoc.pitch; A.pos_unaff = ctx->chunksA * 16;
    A.cov = ctx->d_cov.as<double>(); A.n_covar = ctx->n_covar;
    A.max_iter = max_iter; A.tol = tol; A.out = d_out; A.coef = d_coef;
    const int p = ctx->n_covar + 2;
    const dim3 grid((unsigned)n_variants), block(256);
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
        if (p <= 2) hipLaunchKernelGGL((hpgv::k_logistic<2, 1>), grid, block, 0, st, A);
        else if (p <= 4) hipLaunchKernelGGL((hpgv::k_logistic<4, 1>), grid, block, 0, st, A);
        else if (p <= 6) hipLaunchKernelGGL((hpgv::k_logistic<6, 1>), grid, block, 0, st, A);
        else if (p <= 8) hipLaunchKernelGGL((hpgv::k_logistic<8, 1>), grid, block, 0, st, A);
        else if (p <= 12) hipLaunchKernelGGL((hpgv::k_logistic<12, 2>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((hpgv::k_logistic<16, 4>), grid, block, 0, st, A);
    });
}

// the 1-df chi-square tail as hpgv::chisq_p_value writes it, on libm
double chisq_p_host(double x) {
    if (x != x) return x;
    if (x <= 0.0) return 1.0;
    const double y = x / 2.0;
    const double P = y > 0.5 ? 1.0 - erfc(sqrt(y)) : erf(sqrt(y));
    return 1.0 - P;
}

}  // namespace

extern "C" {

int hpgv_set_covariates(hpgv_ctx *ctx, const double *cov, int n_samples, int n_covar) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_covariates(m_, cov, n_samples, n_covar))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_covar < 0 || (n_covar > 0 && !cov)) return fail(ctx, HPGV_ERR_INVALID, "bad covariates arguments");
    if (n_covar == 0) { ctx->n_covar = 0; ctx->lin_cov.clear(); return linear_image_rebuild(ctx); }
    const Layout &L = ctx->assoc;
    if (n_samples != L.n_samples) return fail(ctx, HPGV_ERR_INVALID, "covariates for %d samples: the cohort has %d columns", n_samples, L.n_samples);
    if (n_covar > HPGV_LOGISTIC_MAX_COVAR) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d covariates: at most %d", n_covar, (int)HPGV_LOGISTIC_MAX_COVAR);
    std::vector<double> laid((size_t)n_covar * L.pitch, 0.0);
    for (size_t pos = 0; pos < L.pitch; ++pos) {
        const int32_t j = L.col_of_pos[pos];
        if (j < 0) continue;
        for (int k = 0; k < n_covar; ++k) {
            const double c = cov[(size_t)j * (size_t)n_covar + (size_t)k];
            if (!std::isfinite(c)) return fail(ctx, HPGV_ERR_INVALID, "covariate %d of column %d is not finite", k, (int)j);
            laid[(size_t)k * L.pitch + pos] = c;
        }
    }
    DeviceGuard g(ctx->device);
    ctx->n_covar = 0;
    {
        const hipError_t e = ctx->d_cov.reserve(laid.size() * sizeof(double));
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, HPGV_ERR_NOMEM, "the covariates (%zu bytes) do not fit the device", laid.size() * sizeof(double)); }
        HIPCHK(ctx, e);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_cov.p, laid.data(), laid.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->n_covar = n_covar;
    ctx->lin_cov.assign(cov, cov + (size_t)n_samples * (size_t)n_covar);      // the linear model's image follows the covariates
    return linear_image_rebuild(ctx);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_logistic_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int max_iter, double tol,
                            hpgv_logistic_result *d_out, double *d_coef, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (const int rc = logistic_args_check(ctx, max_iter, tol)) return rc;
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_out))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_logistic arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_coef & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_out must be 16-byte aligned, d_coef 8-byte aligned");
    DeviceGuard g(ctx->device);
    return logistic_launch(ctx, d_gt, n_variants, max_iter, tol, d_out, d_coef, (hipStream_t)stream);
}

int hpgv_assoc_logistic(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int max_iter, double tol,
                        hpgv_logistic_result *out, double *coef) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_logistic(m_, gt, pitch, n_variants, max_iter, tol, out, coef))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (const int rc0 = logistic_args_check(ctx, max_iter, tol)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !out))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_logistic arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    return regression_finish(ctx, s, S, out, coef, logistic_launch, max_iter, tol);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_logistic_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                             uint64_t *line_off, uint32_t *field_off, int32_t *status, int max_iter, double tol,
                             hpgv_logistic_result *out, double *coef) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_logistic_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, max_iter, tol, out, coef))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (const int rc0 = logistic_args_check(ctx, max_iter, tol)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !out)) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_logistic_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S))) return rc;
    return regression_finish(ctx, s, S, out, coef, logistic_launch, max_iter, tol);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only: no GPU call, usable without a device ------------------------------------------------------------- */

int hpgv_logistic_fit(const uint8_t *cls, const uint8_t *y, const double *cov, int n, int n_covar, int max_iter, double tol,
                      hpgv_logistic_result *out, double *coef) {
    if (n < 0 || n_covar < 0 || n_covar > HPGV_LOGISTIC_MAX_COVAR || !out || (n > 0 && (!cls || !y || (n_covar > 0 && !cov)))) return HPGV_ERR_INVALID;
    if (max_iter < 1 || max_iter > 100 || !(tol >= 0.0) || !std::isfinite(tol)) return HPGV_ERR_INVALID;
    constexpr int LD = hpgv::LOGIT_LD, MAXP = hpgv::LOGIT_MAXP;
    const int p = n_covar + 2;
    double beta[MAXP] = {0.0}, u[MAXP], D[MAXP], H[MAXP * LD], X[MAXP * LD], V[MAXP * LD], x[MAXP];
    int status = HPGV_LOGIT_OK, iters = 0, n_obs = 0;
    bool converged = false;
    for (int it = 0; it < max_iter; ++it) {
        for (int i = 0; i < p; ++i) { u[i] = 0.0; for (int j = 0; j < p; ++j) H[i * LD + j] = 0.0; }
        n_obs = 0;
        for (int s = 0; s < n; ++s) {
            if (cls[s] > 2) continue;
            ++n_obs;
            x[0] = 1.0; x[1] = (double)cls[s];
            for (int k = 0; k < n_covar; ++k) x[2 + k] = cov[(size_t)s * (size_t)n_covar + (size_t)k];
            double eta = beta[0];
            for (int i = 1; i < p; ++i) eta = fma(beta[i], x[i], eta);
            double w, r;
            hpgv::logit_weights(eta, y[s] ? 1.0 : 0.0, &w, &r);
            for (int i = 0; i < p; ++i) {
                const double t = w * x[i];
                for (int j = i; j < p; ++j) H[i * LD + j] = fma(t, x[j], H[i * LD + j]);
                u[i] = fma(r, x[i], u[i]);
            }
        }
        for (int i = 0; i < p; ++i) { D[i] = H[i * LD + i]; for (int j = 0; j < i; ++j) H[i * LD + j] = H[j * LD + i]; }
        if (hpgv::logit_chol_inv(p, H, X, V, D, 0, 1, [] {})) { status = HPGV_LOGIT_SINGULAR; break; }
        double md = 0.0;
        bool finite = true;
        for (int i = 0; i < p; ++i) {
            double d = 0.0;
            for (int j = 0; j < p; ++j) d = fma(V[i * LD + j], u[j], d);
            beta[i] += d;
            md = fabs(d) > md ? fabs(d) : md;
            finite = finite && std::isfinite(beta[i]);
        }
        iters = it + 1;
        if (!finite) { status = HPGV_LOGIT_NOT_CONVERGED; break; }
        if (md <= tol) { converged = true; break; }
    }
    if (!converged && status == HPGV_LOGIT_OK) status = HPGV_LOGIT_NOT_CONVERGED;
    const bool ok = status == HPGV_LOGIT_OK;
    const double nan = std::nan("");
    out->beta = ok ? beta[1] : nan;
    out->se = ok ? sqrt(V[LD + 1]) : nan;
    const double z = out->beta / out->se;
    out->stat = ok ? z * z : nan;
    out->p = chisq_p_host(out->stat);
    out->n_obs = n_obs; out->iters = iters; out->status = status; out->pad = 0;
    if (coef)
        for (int i = 0; i < p; ++i) { coef[i] = ok ? beta[i] : nan; coef[p + i] = ok ? sqrt(V[i * (LD + 1)]) : nan; }
    return HPGV_OK;
}

}  // extern "C"
