// hpgv_logistic_kernels.h -- logistic regression of the phenotype on the ALT allele count and the covariates of a context, one
// fit per row of the resident assoc-layout matrix (include/hpgv.h "Logistic regression"; PLINK's --logistic --covar).
//
// k_logistic<P, DEAL>: one workgroup of four waves per row, the whole Newton iteration inside the launch.  P is p = C + 2
// padded to a shipped size (the pad coordinates are zero columns that are summed and never read); per iteration
//   1. every lane walks its samples -- two adjacent positions per step: one 16-byte load per covariate row, one 2-byte load of the
//      genotypes -- and adds w x x^T (upper triangle, P (P + 1) / 2 entries) and (y - mu) x (P entries) into registers.  beta is
//      wave-uniform and sits in scalar registers.  A pad, a missing genotype or a position past the row adds w = 0 and y - mu = 0;
//   2. the NE = P (P + 3) / 2 sums of a lane exceed the 256 vector registers a VALU instruction can name from P = 12 on (NE = 90
//      doubles at 12, 152 at 16), so the ENTRIES are dealt to DEAL groups of waves (entry e belongs to group e mod DEAL) and the
//      samples to the 4 / DEAL waves of a group: DEAL = 1 four sample quarters with every entry, DEAL = 4 every wave all samples
//      and a quarter of the entries (eta, exp and the weights are then computed four times over);
//   3. lanes are added by DPP inside a row of 16 and the four rows in the order (0 + 1) + (2 + 3), waves through LDS in wave
//      order: one fixed tree, no atomics;
//   4. logit_chol_inv -- the function the host fit compiles too -- factors H, inverts it and the step follows, all in LDS with the
//      workgroup's 256 threads as its lanes.
// Registers and scratch of the shipped instantiations: DESIGN.md "Logistic regression".
#pragma once
#include "../../include/hpgv.h"
#include "hpgv_kernels.h"

namespace hpgv {

constexpr int LOGIT_MAXP = HPGV_LOGISTIC_MAX_COVAR + 2;
constexpr int LOGIT_LD = 16;                      // row stride of the p x p work matrices
constexpr double LOGIT_PIVOT_EPS = 1e-12;
static_assert(LOGIT_MAXP <= LOGIT_LD, "a work matrix row holds p doubles");

// index of entry (i, j), i <= j, in the row-major upper triangle of a P x P matrix
__host__ __device__ constexpr int logit_tri(int P, int i, int j) { return i * P - i * (i - 1) / 2 + (j - i); }

// mu, then the weight and the residual of one observation
__host__ __device__ inline void logit_weights(double eta, double y, double *w, double *r) {
    const double mu = 1.0 / (1.0 + exp(-eta));
    *w = mu * (1.0 - mu);
    *r = y - mu;
}

// H = L L^T, X = L^-1, V = X^T X = H^-1 for the leading p x p of A (lower triangle read, overwritten by L), all three with
// row stride LOGIT_LD; D: the diagonal of H as it was.  Returns 1 at the first pivot <= LOGIT_PIVOT_EPS * D[k] (or NaN).
// `lane` of `nl` lanes work side by side and meet in sync(); every element sees the same operations in the same order whatever
// nl is, so one host thread (nl = 1, a sync that does nothing) and a workgroup give the same bits.
template <class Sync>
__host__ __device__ inline int logit_chol_inv(int p, double *A, double *X, double *V, const double *D, int lane, int nl, Sync sync) {
    for (int k = 0; k < p; ++k) {
        sync();
        const double d = A[k * LOGIT_LD + k];
        if (!(d > LOGIT_PIVOT_EPS * D[k])) return 1;
        const double r = sqrt(d);
        sync();                                   // every lane has read the pivot before it becomes L_kk
        for (int i = k + lane; i < p; i += nl) A[i * LOGIT_LD + k] = i == k ? r : A[i * LOGIT_LD + k] / r;
        sync();
        const int m = p - k - 1;
        for (int t = lane; t < m * m; t += nl) {
            const int i = k + 1 + t / m, j = k + 1 + t % m;
            if (j <= i) A[i * LOGIT_LD + j] = fma(-A[i * LOGIT_LD + k], A[j * LOGIT_LD + k], A[i * LOGIT_LD + j]);
        }
    }
    sync();
    for (int j = lane; j < p; j += nl)            // column j of L^-1 by forward substitution
        for (int i = j; i < p; ++i) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s = fma(-A[i * LOGIT_LD + k], X[k * LOGIT_LD + j], s);
            X[i * LOGIT_LD + j] = s / A[i * LOGIT_LD + i];
        }
    sync();
    for (int t = lane; t < p * p; t += nl) {
        const int i = t / p, j = t % p;
        double s = 0.0;
        for (int k = i > j ? i : j; k < p; ++k) s = fma(X[k * LOGIT_LD + i], X[k * LOGIT_LD + j], s);
        V[i * LOGIT_LD + j] = s;
    }
    sync();
    return 0;
}

struct LogitArgs {
    const uint8_t *gt; size_t pitch;              // assoc layout; positions below pos_unaff are affected columns (or their pads)
    int pos_unaff;
    const double *cov; int n_covar;               // n_covar rows of `pitch` doubles
    int max_iter; double tol;
    hpgv_logistic_result *out; double *coef;
};

template <int CTRL>
__device__ __forceinline__ double logit_dpp(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double logit_readlane(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// the wave's sum, the same in every lane: pairs, quads, halves and rows of 16 by DPP, then the four rows (0 + 1) + (2 + 3)
__device__ __forceinline__ double logit_wave_sum(double v) {
    v += logit_dpp<0xB1>(v);      // quad_perm [1,0,3,2]
    v += logit_dpp<0x4E>(v);      // quad_perm [2,3,0,1]
    v += logit_dpp<0x141>(v);     // row_half_mirror
    v += logit_dpp<0x140>(v);     // row_mirror
    return (logit_readlane(v, 0) + logit_readlane(v, 16)) + (logit_readlane(v, 32) + logit_readlane(v, 48));
}
__device__ __forceinline__ double logit_uniform(double v) { return logit_readlane(v, 0); }

// one pass over the samples of subset `sub` for the entries of group G: red[e] = this wave's sum of entry e, *cnt its observations
template <int P, int DEAL, int G>
__device__ __forceinline__ void logit_pass(const LogitArgs &A, const uint8_t *__restrict__ row, const double *s_beta, int sub, int lane,
                                           double *red, int *cnt) {
    constexpr int NH = P * (P + 1) / 2, NE = NH + P, NA = (NE - G + DEAL - 1) / DEAL, NSUB = 4 / DEAL;
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] = 0.0;
    double b[P];
#pragma unroll
    for (int i = 0; i < P; ++i) b[i] = logit_uniform(s_beta[i]);
    int n = 0;
    const size_t pairs = A.pitch / 2;             // the pitch is a multiple of 16
    for (size_t q = (size_t)sub * 64 + (size_t)lane; q < pairs; q += 64 * NSUB) {
        const size_t pos = 2 * q;
        const unsigned g2 = *reinterpret_cast<const unsigned short *>(row + pos);
        double2 c[P - 2 > 0 ? P - 2 : 1];
#pragma unroll
        for (int k = 0; k < P - 2; ++k)
            c[k] = k < A.n_covar ? *reinterpret_cast<const double2 *>(A.cov + (size_t)k * A.pitch + pos) : make_double2(0.0, 0.0);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned byte = (g2 >> (8 * h)) & 0xFFu, lo = byte & 15u, hi = byte >> 4;
            const bool valid = lo != 15u && hi != 15u;
            double x[P];
            x[0] = 1.0;
            x[1] = (double)((lo != 0u) + (hi != 0u));
#pragma unroll
            for (int k = 0; k < P - 2; ++k) x[2 + k] = h ? c[k].y : c[k].x;
            double eta = b[0];
#pragma unroll
            for (int i = 1; i < P; ++i) eta = fma(b[i], x[i], eta);
            double w, r;
            logit_weights(eta, pos + h < (size_t)A.pos_unaff ? 1.0 : 0.0, &w, &r);
            if (!valid) { w = 0.0; r = 0.0; }
            n += valid;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const double t = w * x[i];
#pragma unroll
                for (int j = i; j < P; ++j) {
                    const int e = logit_tri(P, i, j);
                    if (e % DEAL == G) acc[e / DEAL] = fma(t, x[j], acc[e / DEAL]);
                }
            }
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int e = NH + i;
                if (e % DEAL == G) acc[e / DEAL] = fma(r, x[i], acc[e / DEAL]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const double s = logit_wave_sum(acc[a]);
        if (lane == 0) red[a * DEAL + G] = s;
    }
    if (G == 0) {
        const int total = wave_sum(n);
        if (lane == 0) *cnt = total;
    }
}

template <int P, int DEAL>
__global__ __launch_bounds__(256) void k_logistic(LogitArgs A) {
    static_assert(P >= 2 && P <= LOGIT_MAXP && (DEAL == 1 || DEAL == 2 || DEAL == 4), "shipped shapes");
    constexpr int NH = P * (P + 1) / 2, NE = NH + P, NSUB = 4 / DEAL;
    __shared__ double s_red[NSUB][NE];
    __shared__ double s_A[P * LOGIT_LD], s_X[P * LOGIT_LD], s_V[P * LOGIT_LD];
    __shared__ double s_u[P], s_D[P], s_beta[P], s_delta[P];
    __shared__ int s_cnt[NSUB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = wave % DEAL, sub = wave / DEAL;
    const int p = A.n_covar + 2;
    const uint8_t *row = A.gt + (size_t)blockIdx.x * A.pitch;
    if (tid < P) s_beta[tid] = 0.0;
    int status = HPGV_LOGIT_OK, iters = 0, n_obs = 0;
    bool converged = false;
    for (int it = 0; it < A.max_iter; ++it) {
        __syncthreads();                          // beta is written, the partial sums of the last pass are read
        if (grp == 0) logit_pass<P, DEAL, 0>(A, row, s_beta, sub, lane, s_red[sub], &s_cnt[sub]);
        if constexpr (DEAL > 1) if (grp == 1) logit_pass<P, DEAL, 1>(A, row, s_beta, sub, lane, s_red[sub], &s_cnt[sub]);
        if constexpr (DEAL > 2) {
            if (grp == 2) logit_pass<P, DEAL, 2>(A, row, s_beta, sub, lane, s_red[sub], &s_cnt[sub]);
            if (grp == 3) logit_pass<P, DEAL, 3>(A, row, s_beta, sub, lane, s_red[sub], &s_cnt[sub]);
        }
        __syncthreads();
        if (tid < P * P) {                        // the waves' sums in wave order, H mirrored into both triangles
            const int i = tid / P, j = tid % P, e = logit_tri(P, i < j ? i : j, i < j ? j : i);
            double s = s_red[0][e];
#pragma unroll
            for (int q = 1; q < NSUB; ++q) s += s_red[q][e];
            s_A[i * LOGIT_LD + j] = s;
            if (i == j) s_D[i] = s;
        }
        if (tid < P) {
            double s = s_red[0][NH + tid];
#pragma unroll
            for (int q = 1; q < NSUB; ++q) s += s_red[q][NH + tid];
            s_u[tid] = s;
        }
        n_obs = 0;
#pragma unroll
        for (int q = 0; q < NSUB; ++q) n_obs += s_cnt[q];
        __syncthreads();
        if (logit_chol_inv(p, s_A, s_X, s_V, s_D, tid, 256, [] { __syncthreads(); })) { status = HPGV_LOGIT_SINGULAR; break; }
        if (tid < p) {
            double d = 0.0;
            for (int j = 0; j < p; ++j) d = fma(s_V[tid * LOGIT_LD + j], s_u[j], d);
            s_delta[tid] = d;
            s_beta[tid] += d;
        }
        __syncthreads();
        iters = it + 1;
        double md = 0.0;
        bool finite = true;
        for (int i = 0; i < p; ++i) {
            const double a = fabs(s_delta[i]);
            md = a > md ? a : md;
            finite = finite && isfinite(s_beta[i]);
        }
        if (!finite) { status = HPGV_LOGIT_NOT_CONVERGED; break; }
        if (md <= A.tol) { converged = true; break; }
    }
    if (!converged && status == HPGV_LOGIT_OK) status = HPGV_LOGIT_NOT_CONVERGED;
    const bool ok = status == HPGV_LOGIT_OK;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (tid == 0) {
        hpgv_logistic_result r;
        r.beta = ok ? s_beta[1] : nan;
        r.se = ok ? sqrt(s_V[LOGIT_LD + 1]) : nan;
        const double z = r.beta / r.se;
        r.stat = ok ? z * z : nan;
        r.p = chisq_p_value(r.stat);
        r.n_obs = n_obs; r.iters = iters; r.status = status; r.pad = 0;
        A.out[blockIdx.x] = r;
    }
    if (A.coef && tid < 2 * p) {
        const double v = tid < p ? s_beta[tid] : sqrt(s_V[(tid - p) * (LOGIT_LD + 1)]);
        A.coef[(size_t)blockIdx.x * (size_t)(2 * p) + (size_t)tid] = ok ? v : nan;
    }
}

}  // namespace hpgv
