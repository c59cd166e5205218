// hpgv_linear_capi.hip -- C ABI of the linear regression (include/hpgv.h "Linear regression"): the phenotype of a context and the
// model's device image, the device-resident launch of k_linear, the synchronous entry points on a host batch and on a text --
// built as hpgv_assoc_logistic's are: arguments, a slot, stage_chain / text_front, then the regressions' back half (regression_finish, hpgv_internal.h) -- the host-only fit
// and the t tail.  Behind them, in the same order, the max(T) permutations of the statistic (include/hpgv.h "permutations of the
// linear statistic"): the permutation image of a context, the launch of k_linear_perm_rows and k_linear_perm, the synchronous entry
// points -- the regression's records and the permutation's outputs of one staged batch, the scratch by perm_plan -- and the host fit.
#include "hpgv_internal.h"
#include "hpgv_linear_kernels.h"
#include "hpgv_linear_perm_kernels.h"

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

/* ---- permutations of the linear statistic ---------------------------------------------------------------------------- */

constexpr int kMaxLinPerms = 1 << 20;    // as the label permutations: far below the grid's 65 535 rows of LINPERM_PT

double dot_fma(const double *a, const double *b, size_t n) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s = fma(a[i], b[i], s);
    return s;
}

// v -= Q_k (Q_k . v), one k after the other, each product with what the earlier ones left
void project_out(const std::vector<std::vector<double>> &Qv, int K, double *v, size_t n) {
    for (int k = 0; k < K; ++k) {
        const double *q = Qv[(size_t)k].data();
        const double c = dot_fma(q, v, n);
        for (size_t i = 0; i < n; ++i) v[i] = fma(-c, q[i], v[i]);
    }
}

// The once-per-set-call part of the definition over the cohort positions of n_pos positions in ascending order, col(pos) the
// sample behind a position or -1: the image img[(tile * n_pos + pos) * Q + column] -- tile 0: Q_1 .. Q_C and e, tile 1 + p / 16: E_p
// in column p % 16, zeros elsewhere -- and ss[0] = ss_0, ss[1 + p] = ss_p.  order[p * n_samples + j]: the sample whose residual
// sample j takes, a bijection of the cohort's samples (checked by the caller).  false: the covariates are collinear.
template <class Col>
bool linperm_model(size_t n_pos, Col col, const double *y, const double *cov, int C, const int32_t *order, size_t n_samples, int n_perms,
                   std::vector<double> &img, std::vector<double> &ss) {
    std::vector<size_t> P;
    for (size_t pos = 0; pos < n_pos; ++pos) if (col(pos) >= 0) P.push_back(pos);
    const size_t N = P.size(), tiles = ((size_t)n_perms + 15) / 16;
    img.assign((1 + tiles) * n_pos * Q, 0.0);
    ss.assign((size_t)n_perms + 1, 0.0);
    std::vector<long> idx_of_sample(n_samples, -1);
    for (size_t i = 0; i < N; ++i) idx_of_sample[(size_t)col(P[i])] = (long)i;
    std::vector<std::vector<double>> Qv((size_t)C, std::vector<double>(N));
    std::vector<double> v(N), e(N);
    for (int k = 0; k < C; ++k) {
        double m = 0.0;
        for (size_t i = 0; i < N; ++i) m += cov[(size_t)col(P[i]) * (size_t)C + (size_t)k];
        if (N) m /= (double)N;
        for (size_t i = 0; i < N; ++i) v[i] = cov[(size_t)col(P[i]) * (size_t)C + (size_t)k] - m;
        const double norm0 = dot_fma(v.data(), v.data(), N);
        project_out(Qv, k, v.data(), N);
        const double rem = dot_fma(v.data(), v.data(), N);
        if (!(rem > hpgv::LINPERM_EPS * norm0)) return false;
        const double len = sqrt(rem);
        for (size_t i = 0; i < N; ++i) { Qv[(size_t)k][i] = v[i] / len; img[P[i] * Q + (size_t)k] = Qv[(size_t)k][i]; }
    }
    {
        double m = 0.0;
        for (size_t i = 0; i < N; ++i) m += y[col(P[i])];
        if (N) m /= (double)N;
        for (size_t i = 0; i < N; ++i) e[i] = y[col(P[i])] - m;
        project_out(Qv, C, e.data(), N);
        ss[0] = dot_fma(e.data(), e.data(), N);
        for (size_t i = 0; i < N; ++i) img[P[i] * Q + (size_t)C] = e[i];
    }
    for (int p = 0; p < n_perms; ++p) {
        const int32_t *row = order + (size_t)p * n_samples;
        double m = 0.0;
        for (size_t i = 0; i < N; ++i) { v[i] = e[(size_t)idx_of_sample[(size_t)row[col(P[i])]]]; m += v[i]; }
        if (N) m /= (double)N;
        for (size_t i = 0; i < N; ++i) v[i] -= m;
        project_out(Qv, C, v.data(), N);
        ss[1 + (size_t)p] = dot_fma(v.data(), v.data(), N);
        double *tile = img.data() + (1 + (size_t)p / 16) * n_pos * Q + (size_t)p % 16;
        for (size_t i = 0; i < N; ++i) tile[P[i] * Q] = v[i];
    }
    return true;
}

// every row of `order` maps the samples flagged in `cohort` onto themselves, one to one
bool order_rows_are_bijections(const int32_t *order, const std::vector<uint8_t> &cohort, int n_perms, int *bad_row) {
    const size_t ns = cohort.size();
    std::vector<int32_t> seen(ns, -1);
    for (int p = 0; p < n_perms; ++p) {
        const int32_t *row = order + (size_t)p * ns;
        for (size_t j = 0; j < ns; ++j) {
            if (!cohort[j]) continue;
            const int32_t t = row[j];
            if (t < 0 || (size_t)t >= ns || !cohort[(size_t)t] || seen[(size_t)t] == p) { *bad_row = p; return false; }
            seen[(size_t)t] = p;
        }
    }
    return true;
}

int linperm_state_check(const hpgv_ctx *ctx) {
    if (const int rc = linear_state_check(ctx)) return rc;
    if (ctx->n_linperms <= 0) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_linear_perms has not been called (a new cohort, phenotype or covariates drop the permutations)");
    return HPGV_OK;
}

// the launch on `st`: n_ge and batch_max zeroed, the row pass (one workgroup per 16 rows), the permutation pass (one per 64 rows
// x 128 permutations).  d_rows: n_variants x {mu, D} of scratch
int linperm_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_skip, double *d_rows, double *d_t_obs, int32_t *d_n_ge,
                   double *d_batch_max, double *d_perm_t, hipStream_t st) {
    HIPCHK(ctx, hipMemsetAsync(d_batch_max, 0, (size_t)ctx->n_linperms * sizeof(double), st));
    if (n_variants == 0) return HPGV_OK;
    if (ctx->assoc.pitch % 16) return fail(ctx, HPGV_ERR_UNSUPPORTED, "the linear regression needs a row pitch that is a multiple of 16");
    HIPCHK(ctx, hipMemsetAsync(d_n_ge, 0, (size_t)n_variants * sizeof(int32_t), st));
    hpgv::LinPermArgs A;
    A.gt = d_gt; A.pitch = ctx->assoc.pitch; A.n_variants = n_variants;
    A.n_cohort = ctx->nA + ctx->nU; A.n_covar = ctx->n_covar;
    A.n_perms = ctx->n_linperms; A.tiles = (A.n_perms + 15) / 16;
    A.img = ctx->d_linperm.as<double>(); A.npos = image_positions(ctx); A.ss = A.img + (size_t)(1 + A.tiles) * A.npos * Q;
    A.skip = d_skip; A.rows = (double2 *)d_rows; A.t_obs = d_t_obs; A.n_ge = d_n_ge; A.batch_max = (unsigned long long *)d_batch_max; A.perm_t = d_perm_t;
    const dim3 rows_grid((unsigned)((n_variants + hpgv::LINEAR_ROWS - 1) / hpgv::LINEAR_ROWS));
    const dim3 grid((unsigned)((n_variants + hpgv::LINPERM_VT - 1) / hpgv::LINPERM_VT), (unsigned)((A.tiles + hpgv::LINPERM_NT - 1) / hpgv::LINPERM_NT));
    // (option "profile": the two kernels' time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
        hipLaunchKernelGGL(hpgv::k_linear_perm_rows, rows_grid, dim3(256), 0, st, A);
        hipLaunchKernelGGL(hpgv::k_linear_perm, grid, dim3(256), 0, st, A);
    });
}

// the back half of hpgv_assoc_linear_perm and hpgv_assoc_linear_perm_text.  On the slot's stream: the skip bytes (host, may be null:
// rows that take no part), k_linear for the records, the two memsets and the two permutation kernels, the copies out, one
// synchronise.  The slot's tail holds {mu, D} and t_obs per row (24 bytes)
int linperm_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, hpgv_linear_result *out, double *t_obs, int32_t *n_ge, double *batch_max) {
    int rc;
    const size_t n = (size_t)S.n, np = (size_t)ctx->n_linperms;
    PermPlan P;
    if ((rc = perm_plan(ctx, s, n, np, skip, 24, &P))) return rc;
    HIPCHK(ctx, s->dbl.reserve_slack(n * sizeof(hpgv_linear_result) + 16));
    hpgv_linear_result *d_out = s->dbl.as<hpgv_linear_result>();
    double *d_rows = (double *)P.d_tail, *d_t_obs = d_rows + 2 * n;
    if ((rc = linear_launch(ctx, S.d_laid, S.n, d_out, nullptr, s->stream))) return rc;
    if ((rc = linperm_launch(ctx, S.d_laid, S.n, P.d_skip, d_rows, d_t_obs, P.d_n_ge, P.d_max, nullptr, s->stream))) return rc;
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(out, d_out, n * sizeof(hpgv_linear_result), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(t_obs, d_t_obs, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(n_ge, P.d_n_ge, n * 4, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(batch_max, P.d_max, np * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

}  // namespace

// the image of the context's phenotype and covariates, or nothing without a phenotype
int linear_image_rebuild(hpgv_ctx *ctx) {
    ctx->n_linperms = 0;                                   // the permutation image belongs to the model it was made for
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
    if (!y) { ctx->has_pheno = false; ctx->n_linperms = 0; ctx->lin_y.clear(); return HPGV_OK; }
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

/* ---- permutations of the linear statistic ---------------------------------------------------------------------------- */

int hpgv_set_linear_perms(hpgv_ctx *ctx, const int32_t *order, int n_perms) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_linear_perms(m_, order, n_perms))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = linear_state_check(ctx)) return rc0;
    if (n_perms < 0 || (n_perms > 0 && !order)) return fail(ctx, HPGV_ERR_INVALID, "bad linear_perms arguments");
    if (n_perms > kMaxLinPerms) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d permutations: at most %d per call", n_perms, kMaxLinPerms);
    ctx->n_linperms = 0;
    if (n_perms == 0) return HPGV_OK;
    const Layout &L = ctx->assoc;
    std::vector<uint8_t> cohort((size_t)L.n_samples, 0);
    for (size_t pos = 0; pos < L.pitch; ++pos) if (L.col_of_pos[pos] >= 0) cohort[(size_t)L.col_of_pos[pos]] = 1;
    int bad = 0;
    if (!order_rows_are_bijections(order, cohort, n_perms, &bad)) return fail(ctx, HPGV_ERR_INVALID, "row %d of the order is not a bijection of the cohort columns", bad);
    const size_t n_pos = image_positions(ctx);
    std::vector<double> img, ss;
    if (!linperm_model(n_pos, [&](size_t pos) { return pos < L.pitch ? (long)L.col_of_pos[pos] : -1L; }, ctx->lin_y.data(), ctx->lin_cov.data(), ctx->n_covar,
                       order, (size_t)L.n_samples, n_perms, img, ss))
        return fail(ctx, HPGV_ERR_INVALID, "the covariates are collinear: no permutations of the linear statistic");
    DeviceGuard g(ctx->device);
    const size_t bytes = (img.size() + ss.size()) * sizeof(double);
    const hipError_t e = ctx->d_linperm.reserve(bytes);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, HPGV_ERR_NOMEM, "the permutation image (%zu bytes) does not fit the device", bytes); }
    HIPCHK(ctx, e);
    HIPCHK(ctx, hipMemcpy(ctx->d_linperm.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->d_linperm.as<double>() + img.size(), ss.data(), ss.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->n_linperms = n_perms;
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_linear_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, double *d_t_obs, int32_t *d_n_ge, double *d_batch_max,
                               double *d_perm_t, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = linperm_state_check(ctx)) return rc;
    if (n_variants < 0 || !d_batch_max || (n_variants > 0 && (!d_gt || !d_t_obs || !d_n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_linear_perm arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_t_obs & 7) || ((uintptr_t)d_n_ge & 3) || ((uintptr_t)d_batch_max & 7) || ((uintptr_t)d_perm_t & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt must be 16-byte aligned, d_t_obs, d_batch_max and d_perm_t 8-byte aligned");
    DeviceGuard g(ctx->device);
    // {mu, D} per row: the context's own scratch, grown after the stream that may still read it
    const size_t rows = (size_t)n_variants * 16;
    if (rows) HIPCHK(ctx, ctx->d_linperm_rows.reserve_after_sync((hipStream_t)stream, rows + 16, rows + rows / 4 + 256));
    return linperm_launch(ctx, d_gt, n_variants, nullptr, ctx->d_linperm_rows.as<double>(), d_t_obs, d_n_ge, d_batch_max, d_perm_t, (hipStream_t)stream);
}

int hpgv_assoc_linear_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, hpgv_linear_result *out, double *t_obs, int32_t *n_ge,
                           double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_linear_perm(m_, gt, pitch, n_variants, out, t_obs, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = linperm_state_check(ctx)) return rc0;
    if (n_variants < 0 || !batch_max || (n_variants > 0 && (!gt || !out || !t_obs || !n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_linear_perm arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    return linperm_finish(ctx, s, S, nullptr, out, t_obs, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_linear_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines, uint64_t *line_off,
                                uint32_t *field_off, int32_t *status, hpgv_linear_result *out, double *t_obs, int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_linear_perm_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, out, t_obs, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = linperm_state_check(ctx)) return rc0;
    if (!n_lines || !batch_max || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && (!out || !t_obs || !n_ge)))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_linear_perm_text arguments");
    *n_lines = 0;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if (max_lines > 0 && (rc = text_front_skip(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S))) return rc;
    return linperm_finish(ctx, s, S, K.bytes(), out, t_obs, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_mfma_f64_probe(hpgv_ctx *ctx, int steps, int iters, float *ms, double *flop) {
    ctx = first_member(ctx);
    if (!ctx || !ms || !flop || steps <= 0 || iters <= 0) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    hipEvent_t a, b;
    HIPCHK(ctx, hipEventCreate(&a));
    HIPCHK(ctx, hipEventCreate(&b));
    const unsigned blocks = (unsigned)(ctx->n_cus * 8);      // eight workgroups of four waves per CU
    auto go = [&] { hipLaunchKernelGGL(hpgv::k_mfma_f64_probe, dim3(blocks), dim3(256), 0, nullptr, steps, (double *)ctx->d_sink); };
    go();
    HIPCHK(ctx, hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) go();
    HIPCHK(ctx, hipEventRecord(b, nullptr));
    HIPCHK(ctx, hipEventSynchronize(b));
    float t = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&t, a, b));
    *ms = t / (float)iters;
    *flop = (double)blocks * 4.0 * (double)steps * (double)hpgv::LINPERM_PROBE_ACC * (2.0 * 16 * 16 * 4);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return HPGV_OK;
}

int hpgv_linear_perm_fit(const uint8_t *cls, const double *y, const double *cov, int n, int n_covar, const int32_t *order, int n_perms, double *t_obs,
                         double *t_perm) {
    if (n < 0 || n_covar < 0 || n_covar > HPGV_LOGISTIC_MAX_COVAR || n_perms < 0 || !t_obs || (n_perms > 0 && (!order || !t_perm)) ||
        (n > 0 && (!cls || !y || (n_covar > 0 && !cov))))
        return HPGV_ERR_INVALID;
    for (int s = 0; s < n; ++s) {
        if (!std::isfinite(y[s])) return HPGV_ERR_INVALID;
        for (int k = 0; k < n_covar; ++k) if (!std::isfinite(cov[(size_t)s * (size_t)n_covar + (size_t)k])) return HPGV_ERR_INVALID;
    }
    try {
        int bad = 0;
        if (!order_rows_are_bijections(order, std::vector<uint8_t>((size_t)n, 1), n_perms, &bad)) return HPGV_ERR_INVALID;
        const int C = n_covar, df = n - (C + 2);
        const size_t N = (size_t)n;
        std::vector<double> img, ss;
        if (!linperm_model(N, [](size_t pos) { return (long)pos; }, y, cov, C, order, N, n_perms, img, ss)) return HPGV_ERR_INVALID;
        const double nan = __builtin_nan("");
        int n1 = 0, n2 = 0, n_obs = 0;
        double hd[Q] = {0.0}, hv[Q] = {0.0}, mu, D;
        for (size_t s = 0; s < N; ++s) {
            if (cls[s] > 2) continue;
            ++n_obs; n1 += cls[s] == 1; n2 += cls[s] == 2;
            for (int f = 0; f <= C; ++f) { hd[f] = fma((double)cls[s], img[s * Q + (size_t)f], hd[f]); hv[f] += img[s * Q + (size_t)f]; }
        }
        const bool part = hpgv::linperm_row(C, n_obs, n1, n2, df, hd, hv, &mu, &D);
        *t_obs = part ? hpgv::linperm_t(fma(-mu, hv[C], hd[C]), D, ss[0], df) : nan;
        for (int p = 0; p < n_perms; ++p) {
            if (!part) { t_perm[p] = nan; continue; }
            const double *E = img.data() + (1 + (size_t)p / 16) * N * Q + (size_t)p % 16;
            double sd = 0.0, sv = 0.0;
            for (size_t s = 0; s < N; ++s) {
                if (cls[s] > 2) continue;
                sd = fma((double)cls[s], E[s * Q], sd); sv += E[s * Q];
            }
            t_perm[p] = hpgv::linperm_t(fma(-mu, sv, sd), D, ss[1 + (size_t)p], df);
        }
    } catch (const std::bad_alloc &) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

}  // extern "C"
