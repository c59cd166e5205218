// hpgv_pca_capi.hip -- C ABI of the principal components (include/hpgv.h "PCA"): the GRM's sums as an f64 matrix, the block
// product Y = A Q, the solver (block subspace iteration with Rayleigh-Ritz: the n x L work on the device, the L x L work on the
// host) and the host-only pieces of it: the cyclic Jacobi eigen-solver, the Cholesky factor's inverse, the block width.
#include "hpgv_internal.h"
#include "hpgv_grm_kernels.h"
#include "hpgv_pca_kernels.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace {

constexpr int PCA_MAX_L = 32;

int pca_apply_launch(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, const double *d_Q, int L, double *d_Y, hipStream_t st) {
    const unsigned panels = (unsigned)((n + hpgv::PCA_PANEL - 1) / hpgv::PCA_PANEL);
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
#ifdef HPGV_ABLATION
        if (ctx->pca_apply_vector) {
            if (L == 16) hipLaunchKernelGGL(hpgv::k_pca_apply_vector<16>, dim3(panels), dim3(256), 0, st, d_A, n, lda, d_Q, d_Y);
            else hipLaunchKernelGGL(hpgv::k_pca_apply_vector<32>, dim3(panels), dim3(256), 0, st, d_A, n, lda, d_Q, d_Y);
            return;
        }
#endif
        if (L == 16) hipLaunchKernelGGL(hpgv::k_pca_apply<1>, dim3(panels), dim3(256), 0, st, d_A, n, lda, d_Q, d_Y);
        else hipLaunchKernelGGL(hpgv::k_pca_apply<2>, dim3(panels), dim3(256), 0, st, d_A, n, lda, d_Q, d_Y);
    });
}

// the device side of one solve: three n x L blocks, the Gram partials, two L x L matrices in and one out
struct PcaWork {
    hpgv_ctx *ctx;
    int n, L, chunks;
    double *blk[3] = {nullptr, nullptr, nullptr}, *partial = nullptr, *small = nullptr;      // small: M, M2, C
    hipStream_t st = nullptr;
    PcaWork(hpgv_ctx *c, int n_, int L_) : ctx(c), n(n_), L(L_), chunks((n_ + hpgv::PCA_CHUNK - 1) / hpgv::PCA_CHUNK) {}
    ~PcaWork() {
        for (double *b : blk) if (b) (void)hipFree(b);
        if (partial) (void)hipFree(partial);
        if (small) (void)hipFree(small);
    }
    int alloc() {
        for (double *&b : blk) HIPCHK(ctx, hipMalloc((void **)&b, (size_t)n * L * sizeof(double)));
        HIPCHK(ctx, hipMalloc((void **)&partial, (size_t)chunks * L * L * sizeof(double)));
        HIPCHK(ctx, hipMalloc((void **)&small, (size_t)3 * L * L * sizeof(double)));
        return HPGV_OK;
    }
    // C (host, L x L) = X^T Z
    int gram(const double *X, const double *Z, double *C) {
        if (L == 16) hipLaunchKernelGGL(hpgv::k_pca_gram<16>, dim3((unsigned)chunks), dim3(256), 0, st, X, Z, n, partial);
        else hipLaunchKernelGGL(hpgv::k_pca_gram<32>, dim3((unsigned)chunks), dim3(256), 0, st, X, Z, n, partial);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(hpgv::k_pca_gram_sum, dim3((unsigned)((L * L + 255) / 256)), dim3(256), 0, st, partial, chunks, L * L, small + 2 * L * L);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(C, small + 2 * L * L, (size_t)L * L * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return HPGV_OK;
    }
    // Z = X M, or Z = X M - X2 M2 (M, M2 on the host)
    int rightmul(const double *X, const double *M, const double *X2, const double *M2, double *Z) {
        HIPCHK(ctx, hipMemcpyAsync(small, M, (size_t)L * L * sizeof(double), hipMemcpyHostToDevice, st));
        if (X2) HIPCHK(ctx, hipMemcpyAsync(small + L * L, M2, (size_t)L * L * sizeof(double), hipMemcpyHostToDevice, st));
        const unsigned grid = (unsigned)(((long long)n * L + 255) / 256);
        if (L == 16) hipLaunchKernelGGL(hpgv::k_pca_rightmul<16>, dim3(grid), dim3(256), 0, st, X, small, X2, small + L * L, n, Z);
        else hipLaunchKernelGGL(hpgv::k_pca_rightmul<32>, dim3(grid), dim3(256), 0, st, X, small, X2, small + L * L, n, Z);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st));      // (M and M2 are the caller's stack or vector: done with before it goes on)
        return HPGV_OK;
    }
    // CholQR: to = from R^-1 with from^T from = R^T R
    int cholqr(const double *from, double *to) {
        std::vector<double> G((size_t)L * L), M((size_t)L * L);
        if (const int rc = gram(from, from, G.data())) return rc;
        if (hpgv_pca_chol_inv(L, G.data(), M.data()))
            return fail(ctx, HPGV_ERR_UNSUPPORTED, "a Cholesky pivot of the %d x %d Gram matrix failed: the matrix has rank below %d (or is not finite)", L, L, L);
        return rightmul(from, M.data(), nullptr, nullptr, to);
    }
};

// x (stride 1, length n) to unit 2-norm, its component of largest magnitude positive (the lowest index on a tie)
void pca_normalise(double *x, int n) {
    double ss = 0.0, big = -1.0;
    int at = 0;
    for (int i = 0; i < n; ++i) {
        ss += x[i] * x[i];
        if (fabs(x[i]) > big) { big = fabs(x[i]); at = i; }
    }
    const double nrm = sqrt(ss);
    const double f = (nrm > 0.0 ? 1.0 / nrm : 1.0) * (x[at] < 0.0 ? -1.0 : 1.0);
    for (int i = 0; i < n; ++i) x[i] *= f;
}

// the result's order: of the Ritz pairs by decreasing |theta| the first k, written by decreasing theta (the lower index first on a tie)
void pca_order(const double *theta, int k, int *order) {
    for (int i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order, order + k, [&](int a, int b) { return theta[a] > theta[b]; });
}

// n <= L: Jacobi of the whole matrix on the host
int pca_small(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, int k, double tol, double *eigval, double *vec, double *resid, int *n_iter, int *converged) {
    std::vector<double> A((size_t)n * n), H, theta((size_t)n);
    HIPCHK(ctx, hipMemcpy2D(A.data(), (size_t)n * sizeof(double), d_A, lda * sizeof(double), (size_t)n * sizeof(double), (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            if (!std::isfinite(A[(size_t)i * n + j])) return fail(ctx, HPGV_ERR_UNSUPPORTED, "the matrix is not finite at (%d, %d)", i, j);
    H = A;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) H[(size_t)i * n + j] = H[(size_t)j * n + i] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
    hpgv_pca_jacobi(n, H.data(), theta.data());
    int order[PCA_MAX_L];
    pca_order(theta.data(), k, order);
    double worst = 0.0;
    std::vector<double> x((size_t)n);
    for (int c = 0; c < k; ++c) {
        const int p = order[c];
        for (int i = 0; i < n; ++i) x[i] = H[(size_t)i * n + p];
        pca_normalise(x.data(), n);
        double ss = 0.0;
        for (int i = 0; i < n; ++i) {
            double s = -theta[p] * x[i];
            for (int j = 0; j < n; ++j) s += A[(size_t)i * n + j] * x[j];
            ss += s * s;
        }
        eigval[c] = theta[p];
        resid[c] = sqrt(ss);
        worst = std::max(worst, resid[c]);
        for (int i = 0; i < n; ++i) vec[(size_t)i * k + c] = x[i];
    }
    *n_iter = 0;
    *converged = worst <= tol * fabs(theta[0]) || worst == 0.0;
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_grm_matrix_dev(hpgv_ctx *ctx, const hpgv_grm_acc *d_acc, int n_cols, int frac_bits, double *d_A, size_t lda, uint64_t *d_n_empty, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (frac_bits < 0 || frac_bits > hpgv::GRM_MAX_FRAC_BITS) return fail(ctx, HPGV_ERR_INVALID, "frac_bits %d: 0 .. %d", frac_bits, hpgv::GRM_MAX_FRAC_BITS);
    if (n_cols < 0) return fail(ctx, HPGV_ERR_INVALID, "bad grm_matrix arguments: %d columns", n_cols);
    if (lda < (size_t)n_cols || (lda & 1)) return fail(ctx, HPGV_ERR_INVALID, "lda %zu: at least n_cols %d, and even", lda, n_cols);
    if (!d_n_empty) return fail(ctx, HPGV_ERR_INVALID, "d_n_empty is NULL");
    if (((uintptr_t)d_acc & 15) || ((uintptr_t)d_A & 15) || ((uintptr_t)d_n_empty & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_acc and d_A must be 16-byte aligned, d_n_empty 8-byte aligned");
    if (n_cols > 0 && (!d_acc || !d_A)) return fail(ctx, HPGV_ERR_INVALID, "bad grm_matrix arguments: d_acc and d_A are required");
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(ctx, hipMemsetAsync(d_n_empty, 0, sizeof(uint64_t), st));
    if (n_cols == 0) return HPGV_OK;
    const unsigned T = (unsigned)((n_cols + 31) / 32);
    if (T > 65535u) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d columns: more than 65 535 tiles of 32 exceed the grid", n_cols);
    hipLaunchKernelGGL(hpgv::k_grm_matrix, dim3(T, T), dim3(256), 0, st, reinterpret_cast<const long long *>(d_acc), n_cols, ldexp(1.0, -2 * frac_bits), d_A, lda,
                       reinterpret_cast<unsigned long long *>(d_n_empty));
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_pca_apply_dev(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, const double *d_Q, int L, double *d_Y, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (L != 16 && L != 32) return fail(ctx, HPGV_ERR_INVALID, "L %d: 16 or 32", L);
    if (n < 0) return fail(ctx, HPGV_ERR_INVALID, "bad pca_apply arguments: n %d", n);
    if (lda < (size_t)n || (lda & 1)) return fail(ctx, HPGV_ERR_INVALID, "lda %zu: at least n %d, and even", lda, n);
    if (((uintptr_t)d_A & 15) || ((uintptr_t)d_Q & 7) || ((uintptr_t)d_Y & 7)) return fail(ctx, HPGV_ERR_INVALID, "d_A must be 16-byte aligned, d_Q and d_Y 8-byte aligned");
    if (n == 0) return HPGV_OK;
    if (!d_A || !d_Q || !d_Y) return fail(ctx, HPGV_ERR_INVALID, "bad pca_apply arguments: d_A, d_Q and d_Y are required");
    DeviceGuard g(ctx->device);
    return pca_apply_launch(ctx, d_A, n, lda, d_Q, L, d_Y, (hipStream_t)stream);
}

int hpgv_pca_dev(hpgv_ctx *ctx, const double *d_A, int n, size_t lda, int k, double tol, int max_iter, uint64_t seed, double *eigval, double *vec, double *resid,
                 int *n_iter, int *converged) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!d_A || !eigval || !vec || !resid || !n_iter || !converged) return fail(ctx, HPGV_ERR_INVALID, "bad pca arguments: a NULL pointer");
    if (k < 1 || k > 24 || k > n) return fail(ctx, HPGV_ERR_INVALID, "k %d: 1 .. 24 and at most n %d", k, n);
    if (!(tol > 0.0) || !std::isfinite(tol)) return fail(ctx, HPGV_ERR_INVALID, "tol %g: positive and finite", tol);
    if (max_iter < 1) return fail(ctx, HPGV_ERR_INVALID, "max_iter %d: at least 1", max_iter);
    if (lda < (size_t)n || (lda & 1)) return fail(ctx, HPGV_ERR_INVALID, "lda %zu: at least n %d, and even", lda, n);
    if ((uintptr_t)d_A & 15) return fail(ctx, HPGV_ERR_INVALID, "d_A must be 16-byte aligned");
    *n_iter = 0; *converged = 0;
    DeviceGuard g(ctx->device);
    const int L = hpgv_pca_block(k);
    if (n <= L) return pca_small(ctx, d_A, n, lda, k, tol, eigval, vec, resid, n_iter, converged);

    PcaWork W(ctx, n, L);
    if (const int rc = W.alloc()) return rc;
    double *Q = W.blk[0], *Y = W.blk[1], *Z = W.blk[2];
    hipLaunchKernelGGL(hpgv::k_pca_init, dim3((unsigned)(((long long)n * L + 255) / 256)), dim3(256), 0, W.st, Q, n, L, seed);
    HIPCHK(ctx, hipGetLastError());
    if (const int rc = W.cholqr(Q, Z)) return rc;
    if (const int rc = W.cholqr(Z, Q)) return rc;

    const size_t LL = (size_t)L * L;
    std::vector<double> H(LL), Wm(LL), WT(LL), C(LL), theta((size_t)L);
    for (int it = 1;; ++it) {
        if (const int rc = pca_apply_launch(ctx, d_A, n, lda, Q, L, Y, W.st)) return rc;
        if (const int rc = W.gram(Q, Y, H.data())) return rc;
        for (int a = 0; a < L; ++a)
            for (int b = 0; b <= a; ++b) {
                const double h = 0.5 * (H[(size_t)a * L + b] + H[(size_t)b * L + a]);
                if (!std::isfinite(h)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "the matrix is not finite");
                Wm[(size_t)a * L + b] = Wm[(size_t)b * L + a] = h;
            }
        hpgv_pca_jacobi(L, Wm.data(), theta.data());      // Wm: the Ritz vectors' coefficients in columns, by decreasing |theta|
        for (int a = 0; a < L; ++a)
            for (int b = 0; b < L; ++b) WT[(size_t)a * L + b] = Wm[(size_t)a * L + b] * theta[b];
        if (const int rc = W.rightmul(Y, Wm.data(), Q, WT.data(), Z)) return rc;      // R = Y W - Q W Theta
        if (const int rc = W.gram(Z, Z, C.data())) return rc;
        double worst = 0.0;
        for (int c = 0; c < k; ++c) worst = std::max(worst, sqrt(C[(size_t)c * L + c]));
        const bool done = worst <= tol * fabs(theta[0]);
        if (done || it == max_iter) {
            int order[PCA_MAX_L];
            pca_order(theta.data(), k, order);
            if (const int rc = W.rightmul(Q, Wm.data(), nullptr, nullptr, Z)) return rc;      // the Ritz vectors X = Q W
            std::vector<double> X((size_t)n * L), x((size_t)n);
            HIPCHK(ctx, hipMemcpy(X.data(), Z, (size_t)n * L * sizeof(double), hipMemcpyDeviceToHost));
            for (int c = 0; c < k; ++c) {
                const int p = order[c];
                for (int i = 0; i < n; ++i) x[i] = X[(size_t)i * L + p];
                pca_normalise(x.data(), n);
                for (int i = 0; i < n; ++i) vec[(size_t)i * k + c] = x[i];
                eigval[c] = theta[p];
                resid[c] = sqrt(C[(size_t)p * L + p]);
            }
            *n_iter = it;
            *converged = done ? 1 : 0;
            return HPGV_OK;
        }
        if (const int rc = W.cholqr(Y, Z)) return rc;
        if (const int rc = W.cholqr(Z, Q)) return rc;
    }
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only pieces: no GPU call, usable without a device -------------------------------------------------------------- */

int hpgv_pca_block(int k) { return k < 1 ? -1 : k <= 8 ? 16 : k <= 24 ? 32 : -1; }

// Cyclic Jacobi: sweeps over the pairs p < q in row order, each off-diagonal element above 2^-8 eps ||H||_F / L rotated to zero
// (Rutishauser's tangent form); it ends with the first sweep that rotates nothing, after 64 sweeps at the latest.  Then the pairs
// are put in order of decreasing |theta| (the lower index first among equals).
int hpgv_pca_jacobi(int L, double *H, double *theta) {
    if (L < 1 || L > PCA_MAX_L || !H || !theta) return HPGV_ERR_INVALID;
    double V[PCA_MAX_L * PCA_MAX_L], A[PCA_MAX_L * PCA_MAX_L];
    double nf = 0.0;
    for (int i = 0; i < L; ++i)
        for (int j = 0; j < L; ++j) {
            A[i * L + j] = i == j ? H[i * L + j] : 0.5 * (H[i * L + j] + H[j * L + i]);
            V[i * L + j] = i == j ? 1.0 : 0.0;
            nf += A[i * L + j] * A[i * L + j];
        }
    const double small = DBL_EPSILON * 0x1p-8 * sqrt(nf) / (double)L;
    for (int sweep = 0; sweep < 64; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < L - 1; ++p)
            for (int q = p + 1; q < L; ++q) {
                const double apq = A[p * L + q];
                if (!(fabs(apq) > small)) continue;
                rotated++;
                const double th = (A[q * L + q] - A[p * L + p]) / (2.0 * apq);
                const double t = fabs(th) > 0x1p500 ? 0.5 / th : (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[p * L + p] -= t * apq;
                A[q * L + q] += t * apq;
                A[p * L + q] = A[q * L + p] = 0.0;
                for (int r = 0; r < L; ++r) {
                    if (r != p && r != q) {
                        const double arp = A[r * L + p], arq = A[r * L + q];
                        A[r * L + p] = A[p * L + r] = c * arp - s * arq;
                        A[r * L + q] = A[q * L + r] = s * arp + c * arq;
                    }
                    const double vrp = V[r * L + p], vrq = V[r * L + q];
                    V[r * L + p] = c * vrp - s * vrq;
                    V[r * L + q] = s * vrp + c * vrq;
                }
            }
        if (!rotated) break;
    }
    int order[PCA_MAX_L];
    for (int i = 0; i < L; ++i) order[i] = i;
    std::stable_sort(order, order + L, [&](int a, int b) { return fabs(A[a * L + a]) > fabs(A[b * L + b]); });
    for (int j = 0; j < L; ++j) {
        theta[j] = A[order[j] * L + order[j]];
        for (int i = 0; i < L; ++i) H[i * L + j] = V[i * L + order[j]];
    }
    return HPGV_OK;
}

int hpgv_pca_chol_inv(int L, const double *G, double *M) {
    if (L < 1 || L > PCA_MAX_L || !G || !M) return -1;
    double R[PCA_MAX_L * PCA_MAX_L];
    double top = 0.0;
    for (int i = 0; i < L; ++i) top = std::max(top, G[i * L + i]);
    const double least = (double)L * DBL_EPSILON * top;
    for (int i = 0; i < L * L; ++i) { R[i] = 0.0; M[i] = 0.0; }
    for (int j = 0; j < L; ++j) {
        double d = G[j * L + j];
        for (int m = 0; m < j; ++m) d -= R[m * L + j] * R[m * L + j];
        if (!(d > least)) return 1;                       // (a NaN pivot too)
        const double rjj = sqrt(d);
        R[j * L + j] = rjj;
        for (int i = j + 1; i < L; ++i) {
            double s = 0.5 * (G[j * L + i] + G[i * L + j]);
            for (int m = 0; m < j; ++m) s -= R[m * L + j] * R[m * L + i];
            R[j * L + i] = s / rjj;
        }
    }
    // M = R^-1, upper triangular: column by column, back substitution of R m = e_c
    for (int c = 0; c < L; ++c)
        for (int i = c; i >= 0; --i) {
            double s = i == c ? 1.0 : 0.0;
            for (int m = i + 1; m <= c; ++m) s -= R[i * L + m] * M[m * L + c];
            M[i * L + c] = s / R[i * L + i];
        }
    return 0;
}

}  // extern "C"
