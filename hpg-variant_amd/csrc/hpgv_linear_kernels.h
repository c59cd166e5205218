// hpgv_linear_kernels.h -- linear regression of a quantitative trait on the ALT allele count and the covariates of a context, one
// ordinary least squares fit per row of the resident assoc-layout matrix (include/hpgv.h "Linear regression"; PLINK's --linear
// --covar).
//
// k_linear: one workgroup of four waves owns a tile of 16 rows.
//   1. The dense product h = sum_obs d f on v_mfma_f64_16x16x4_f64 (linear_tile_walk, shared with the permutations' row pass).  Lane (r = lane & 15, kq = lane >> 4) of a wave loads 16
//      genotype bytes of row r at position chunk * 64 + 16 kq with one 16-byte load; MFMA step s of the chunk takes the dosage
//      of byte s as its A operand (missing, pad, a row past the matrix: 0.0) and feature r of position chunk * 64 + 16 kq + s
//      as its B operand: 16 MFMAs per 64 positions, the lanes of one kq read 128 contiguous bytes of the image.  The
//      accumulator (4 doubles per lane) holds h of the 16 rows.  Wave w takes the chunks w, w + 4, ..; the four partial tiles
//      are added through LDS in wave order.  An MFMA output row depends on its own A row only, so neither the tile a row falls
//      in nor a ragged last tile changes a bit of it.
//   2. The class counts are integers from the same bytes (lanes by shuffles, waves through LDS).
//   3. Each wave then finishes four rows of the tile, one after the other, all of it wave-local (no workgroup barrier, so the
//      early return of logit_chol_inv on a bad pivot is one row's own business):
//        the correction of S: the row's bytes again, 1 024 positions per step, a 16-bit mask of flagged positions per lane --
//        the missing ones, or the observed ones where they are fewer -- listed in ascending order by a prefix sum over the
//        lanes and taken in batches of 64 as they fill, whose feature rows go to LDS with 16 independent loads per lane; the
//        q (q + 1) / 2 <= 136 entries of S are dealt to the lanes (at most three each) and take one fma per flagged position,
//        eight positions per turn.  A row without a missing call skips all this;
//        the solve: linear_record, the function the host fit compiles too, with the wave's 64 lanes.
// Registers, LDS and scratch: DESIGN.md "Linear regression".
#pragma once
#include "../../include/hpgv.h"
#include "hpgv_logistic_kernels.h"

namespace hpgv {

constexpr int LINEAR_Q = 16;                       // doubles per position of the feature image, row stride of G and S
constexpr double LINEAR_EXACT_EPS = 1e-12;
static_assert(LOGIT_MAXP <= LINEAR_Q && LOGIT_LD == LINEAR_Q, "one MFMA tile holds every feature column");

/* ---- the t tail ------------------------------------------------------------------------------------------------------ */

// ln B(a, 1/2) = ln Gamma(a) + ln Gamma(1/2) - ln Gamma(a + 1/2) for a >= 1/2: the ratio is carried up to a >= 32 by
// Gamma(a + 1/2) / Gamma(a) = Gamma(a + 3/2) / Gamma(a + 1) * a / (a + 1/2), then Stirling's series of the ratio (next term
// below 1e-17 there).  No lgamma: log is all the host and the device have to agree on.
__host__ __device__ inline double linear_lbeta_half(double a) {
    double prod = 1.0;
    while (a < 32.0) { prod *= a / (a + 0.5); a += 1.0; }
    const double ia = 1.0 / a, i2 = ia * ia;
    const double series = ia * (1.0 / 8.0 - i2 * (1.0 / 192.0 - i2 * (1.0 / 640.0 - i2 * (17.0 / 14336.0 - i2 * (31.0 / 18432.0)))));
    return 0.5723649429247000870717 - (0.5 * log(a) - series) - log(prod);      // ln Gamma(1/2) = ln(pi) / 2
}

// the continued fraction of I_x(a, b) (modified Lentz), for x < (a + 1) / (a + b + 2)
__host__ __device__ inline double linear_betacf(double a, double b, double x) {
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double hh = d;
    for (int m = 1; m <= 20000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        hh *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        hh *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return hh;
}

// two-sided tail of Student's t: I_x(df / 2, 1 / 2), x = df / (df + t^2); through 1 - I_{1-x}(1 / 2, df / 2) where x is large
__host__ __device__ inline double linear_t_p(double t, int df) {
    if (t != t || df < 1) return __builtin_nan("");
    const double a = 0.5 * df, b = 0.5, t2 = t * t;
    if (t2 > 1.7e308) return 0.0;
    const double x = df / (df + t2), y = t2 / (df + t2);
    const double lnx = -log1p(t2 / df), lny = log(y), lb = linear_lbeta_half(a);
    double P;
    if (x < (a + 1.0) / (a + b + 2.0)) P = exp(a * lnx + b * lny - lb) * linear_betacf(a, b, x) / a;
    else P = 1.0 - exp(b * lny + a * lnx - lb) * linear_betacf(b, a, y) / b;
    return P < 0.0 ? 0.0 : P > 1.0 ? 1.0 : P;
}

/* ---- moments -> record ----------------------------------------------------------------------------------------------- */

// The step from a row's moments to its record, on `nl` lanes that meet in sync() (one host thread: nl = 1 and a sync that
// does nothing).  S: the q x q moments of the centred features [1, c_1 .. c_C, y] (full, row stride LINEAR_Q), h: sum_obs d f,
// mean[f]: what feature f was centred by (mean[0] unused).  A, X, V (p rows of LOGIT_LD) and D (p) are work space.  Every lane
// computes the scalars from the shared matrices; lane 0 writes *out, lanes t < 2p write coef[t].
template <class Sync>
__host__ __device__ inline void linear_record(int C, const double *S, const double *h, int n1, int n2, int n_obs, const double *mean,
                                              double *A, double *X, double *V, double *D, int lane, int nl, Sync sync,
                                              hpgv_linear_result *out, double *coef) {
    const int p = C + 2, iy = C + 1, df = n_obs - p;
    const double nan = __builtin_nan("");
    // the normal equations in the order [1, d, c ..]: coefficient i != 1 is feature i ? i - 1 : 0
    for (int t = lane; t < p * p; t += nl) {
        const int i = t / p, j = t % p;
        double v;
        if (i == 1 && j == 1) v = (double)(n1 + 4 * n2);
        else if (i == 1 || j == 1) { const int o = i == 1 ? j : i; v = o == 0 ? (double)(n1 + 2 * n2) : h[o - 1]; }
        else v = S[(i ? i - 1 : 0) * LINEAR_Q + (j ? j - 1 : 0)];
        A[i * LOGIT_LD + j] = v;
        if (i == j) D[i] = v;
    }
    int status = HPGV_LINEAR_OK;
    if (df < 1) status = HPGV_LINEAR_SINGULAR;
    else if (logit_chol_inv(p, A, X, V, D, lane, nl, sync)) status = HPGV_LINEAR_SINGULAR;
    if (status != HPGV_LINEAR_OK) {
        if (lane == 0) { out->beta = out->se = out->stat = out->p = nan; out->n_obs = n_obs; out->df = df; out->status = status; out->pad = 0; }
        if (coef) for (int t = lane; t < 2 * p; t += nl) coef[t] = nan;
        return;
    }
    const double yty = S[iy * LINEAR_Q + iy];
    auto xty = [&](int j) { return j == 1 ? h[iy] : S[(j ? j - 1 : 0) * LINEAR_Q + iy]; };
    auto beta_c = [&](int i) { double s = 0.0; for (int j = 0; j < p; ++j) s = fma(V[i * LOGIT_LD + j], xty(j), s); return s; };     // centred model
    double rss = yty;
    for (int i = 0; i < p; ++i) {
        double z = 0.0;
        for (int j = 0; j <= i; ++j) z = fma(X[i * LOGIT_LD + j], xty(j), z);
        rss = fma(-z, z, rss);
    }
    if (rss <= LINEAR_EXACT_EPS * yty) status = HPGV_LINEAR_EXACT;
    const bool exact = status == HPGV_LINEAR_EXACT;
    const double sigma2 = exact ? 0.0 : rss / (double)df;
    if (lane == 0) {
        const double b1 = beta_c(1), se1 = sqrt(sigma2 * V[LOGIT_LD + 1]), st = exact ? nan : b1 / se1;
        out->beta = b1; out->se = exact ? 0.0 : se1; out->stat = st; out->p = exact ? nan : linear_t_p(st, df);
        out->n_obs = n_obs; out->df = df; out->status = status; out->pad = 0;
    }
    if (coef)
        for (int t = lane; t < 2 * p; t += nl) {
            const int i = t < p ? t : t - p;
            double v;
            if (t < p) {
                v = beta_c(i);
                if (i == 0) {                             // the intercept of the un-centred model
                    v += mean[iy];
                    for (int k = 2; k < p; ++k) v = fma(-beta_c(k), mean[k - 1], v);
                }
            } else if (exact) v = 0.0;
            else if (i == 0) {                            // a^T V a, a = (1, 0, -m_1 .. -m_C)
                double q = 0.0;
                for (int r = 0; r < p; ++r) {
                    if (r == 1) continue;
                    double row = V[r * LOGIT_LD];
                    for (int k = 2; k < p; ++k) row = fma(-V[r * LOGIT_LD + k], mean[k - 1], row);
                    q = fma(r == 0 ? 1.0 : -mean[r - 1], row, q);
                }
                v = sqrt(sigma2 * q);
            } else v = sqrt(sigma2 * V[i * (LOGIT_LD + 1)]);
            coef[t] = v;
        }
}

// (i, j), i <= j, of entry e in the row-major upper triangle of a q x q matrix
__host__ __device__ inline void linear_tri_ij(int q, int e, int *i, int *j) {
    int r = 0;
    while (e >= q - r) { e -= q - r; ++r; }
    *i = r; *j = r + e;
}

struct LinArgs {
    const uint8_t *gt; size_t pitch; int n_variants;   // assoc layout
    int nA, segA, nU;                                  // cohort positions: [0, nA) and [segA, segA + nU)
    int n_covar;
    const double *feat;                                // round_up(pitch, 64) positions x LINEAR_Q doubles
    const double *G, *mean;                            // LINEAR_Q x LINEAR_Q, LINEAR_Q
    hpgv_linear_result *out; double *coef;
};

typedef double lin_d4 __attribute__((ext_vector_type(4)));

// LDS operations of one wave are in order; this keeps the compiler from moving them across the point where lanes trade values
__device__ __forceinline__ void linear_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// class of an HPGV8 byte: 0 / 1 / 2, 3 = missing (either nibble 0xF: a pad byte too)
__device__ __forceinline__ unsigned linear_class(unsigned byte) {
    const unsigned lo = byte & 15u, hi = byte >> 4;
    return (lo == 15u || hi == 15u) ? 3u : (unsigned)(lo != 0u) + (unsigned)(hi != 0u);
}

constexpr int LINEAR_ROWS = 16, LINEAR_BATCH = 64, LINEAR_SCAN = 1024;

// The tile walk of a workgroup of four waves over the 16 rows from row0 on (k_linear's step 1 and 2, and the row pass of the
// permutations, hpgv_linear_perm_kernels.h): wave `wave` takes the chunks of 64 positions wave, wave + 4, ..; lane (r, kq) loads the
// 16 bytes of row row0 + r at chunk * 64 + 16 kq, and MFMA step s takes the dosage of byte s as A and image column r of that
// position as B.  acc: the wave's part of sum_obs d f; with VALID accv: its part of sum_obs f, the same steps with A = 1.0 on an
// observed call; c0, c1, c2: the lane's class counts.  `feat`: 16 doubles per position, padded to whole chunks of 64.
template <bool VALID>
__device__ __forceinline__ void linear_tile_walk(const uint8_t *gt, size_t pitch, int n_variants, int row0, const double *feat, int wave, int lane,
                                                 lin_d4 &acc, lin_d4 &accv, int &c0, int &c1, int &c2) {
    const int r = lane & 15, kq = lane >> 4;
    const bool row_ok = row0 + r < n_variants;
    const uint8_t *rp = gt + (size_t)(row_ok ? row0 + r : row0) * pitch;
    for (size_t base = (size_t)wave * 64; base < pitch; base += 256) {
        const size_t pos = base + 16 * (size_t)kq;
        uint4 g = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (row_ok && pos < pitch) g = *reinterpret_cast<const uint4 *>(rp + pos);     // (the pitch is a multiple of 16)
        const double *fp = feat + pos * LINEAR_Q + r;                                     // (the image is padded to 64 positions)
        double f[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) f[s] = fp[s * LINEAR_Q];
        const unsigned w4[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const unsigned cls = linear_class((w4[s >> 2] >> (8 * (s & 3))) & 0xFFu);
            c0 += cls == 0u; c1 += cls == 1u; c2 += cls == 2u;
            const double d = cls == 3u ? 0.0 : (double)cls;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(d, f[s], acc, 0, 0, 0);
            if constexpr (VALID) accv = __builtin_amdgcn_mfma_f64_16x16x4f64(cls == 3u ? 0.0 : 1.0, f[s], accv, 0, 0, 0);
        }
    }
}

__global__ __launch_bounds__(256) void k_linear(LinArgs A) {
    // per wave: the feature rows of a batch of flagged positions (64 x 16 doubles), afterwards the solve's A, X, V (3 x 2 KiB)
    // and the row's S (2 KiB); before either, the waves' partial h tiles (4 doubles x 64 lanes each)
    __shared__ double s_work[4][LINEAR_BATCH * LINEAR_Q];
    __shared__ double s_h[LINEAR_ROWS][LINEAR_Q];
    __shared__ double s_D[4][LINEAR_Q];
    __shared__ int s_list[4][LINEAR_SCAN + LINEAR_BATCH];
    __shared__ int s_cnt[4][LINEAR_ROWS][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * LINEAR_ROWS;
    const size_t pitch = A.pitch;
    const int C = A.n_covar, q = C + 2, p = C + 2;

    /* 1, 2: the product and the counts */
    {
        lin_d4 acc = {0.0, 0.0, 0.0, 0.0}, unused = acc;
        int c0 = 0, c1 = 0, c2 = 0;
        linear_tile_walk<false>(A.gt, pitch, A.n_variants, row0, A.feat, wave, lane, acc, unused, c0, c1, c2);
        c0 += __shfl_xor(c0, 16, 64); c1 += __shfl_xor(c1, 16, 64); c2 += __shfl_xor(c2, 16, 64);
        c0 += __shfl_xor(c0, 32, 64); c1 += __shfl_xor(c1, 32, 64); c2 += __shfl_xor(c2, 32, 64);
        if (kq == 0) { s_cnt[wave][r][0] = c0; s_cnt[wave][r][1] = c1; s_cnt[wave][r][2] = c2; }
#pragma unroll
        for (int t = 0; t < 4; ++t) s_work[wave][t * 64 + lane] = acc[t];
        __syncthreads();
        {   // output row m = 4 t + kq, column r of a wave's tile lies at [t * 64 + lane]; the waves in wave order
            const int m = tid >> 4, c = tid & 15, at = (m >> 2) * 64 + (m & 3) * 16 + c;
            s_h[m][c] = ((s_work[0][at] + s_work[1][at]) + s_work[2][at]) + s_work[3][at];
        }
        __syncthreads();
    }

    /* 3: four rows per wave */
    double *W = s_work[wave], *sA = W, *sX = W + 256, *sV = W + 512, *sS = W + 768;
    int *list = s_list[wave];
    const int ne = q * (q + 1) / 2;
    int ei[3], ej[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        ei[t] = ej[t] = 0;
        if (lane + 64 * t < ne) linear_tri_ij(q, lane + 64 * t, &ei[t], &ej[t]);
    }
    for (int m = wave * 4; m < wave * 4 + 4; ++m) {
        const int row = row0 + m;
        if (row >= A.n_variants) break;                   // (wave-uniform)
        int n0 = 0, n1 = 0, n2 = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { n0 += s_cnt[w][m][0]; n1 += s_cnt[w][m][1]; n2 += s_cnt[w][m][2]; }
        const int n_obs = n0 + n1 + n2, n_miss = A.nA + A.nU - n_obs;
        const bool direct = n_miss > n_obs;               // sum the observed positions instead of taking the missing ones from G
        double acc[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = (!direct && lane + 64 * t < ne) ? A.G[ei[t] * LINEAR_Q + ej[t]] : 0.0;
        linear_wave_sync();                               // the last row's solve has read W
        if (n_miss > 0) {
            const uint8_t *rp = A.gt + (size_t)row * pitch;
            const double sign = direct ? 1.0 : -1.0;
            int n_list = 0;                               // positions listed and not yet taken (wave-uniform)
            auto take = [&](int b0, int nb) {             // one batch: list[b0 .. b0 + nb), nb <= LINEAR_BATCH
                linear_wave_sync();                       // the list is written, the last batch is read
#pragma unroll
                for (int it = 0; it < 16; ++it) {         // 4 positions per step, 128 contiguous bytes each; zeros behind the batch
                    const int k = it * 4 + kq;
                    double v = 0.0;
                    if (k < nb) v = A.feat[(size_t)list[b0 + k] * LINEAR_Q + r];
                    W[k * LINEAR_Q + r] = v;
                }
                linear_wave_sync();
                for (int k0 = 0; k0 < nb; k0 += 8) {      // (a zero row adds nothing)
#pragma unroll
                    for (int k = k0; k < k0 + 8; ++k)
#pragma unroll
                        for (int t = 0; t < 3; ++t)
                            if (lane + 64 * t < ne) acc[t] = fma(sign * W[k * LINEAR_Q + ei[t]], W[k * LINEAR_Q + ej[t]], acc[t]);
                }
            };
            for (size_t base = 0; base < pitch; base += LINEAR_SCAN) {
                const size_t pos = base + 16 * (size_t)lane;
                unsigned mask = 0;
                if (pos < pitch) {
                    const uint4 g = *reinterpret_cast<const uint4 *>(rp + pos);
                    const unsigned w4[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const int at = (int)pos + s;
                        const bool cohort = at < A.nA || (at >= A.segA && at < A.segA + A.nU);
                        const bool missing = linear_class((w4[s >> 2] >> (8 * (s & 3))) & 0xFFu) == 3u;
                        if (cohort && missing != direct) mask |= 1u << s;
                    }
                }
                // the step's flagged positions behind those listed, in ascending order: a lane's own behind those of the lanes below it
                const int cnt = __popc(mask);
                int pre = cnt;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const int below = __shfl_up(pre, o, 64); if (lane >= o) pre += below; }
                const int total = __shfl(pre, 63, 64);
                if (total == 0) continue;                 // (wave-uniform)
                int at = n_list + pre - cnt;
                for (unsigned mk = mask; mk; mk &= mk - 1) list[at++] = (int)pos + __builtin_ctz(mk);
                n_list += total;
                int b0 = 0;
                for (; n_list - b0 >= LINEAR_BATCH; b0 += LINEAR_BATCH) take(b0, LINEAR_BATCH);
                if (b0) {                                 // what is left, fewer than a batch, to the front
                    linear_wave_sync();
                    const int left = lane < n_list - b0 ? list[b0 + lane] : 0;
                    linear_wave_sync();
                    if (lane < n_list - b0) list[lane] = left;
                    n_list -= b0;
                }
            }
            if (n_list) take(0, n_list);
            linear_wave_sync();                           // W is read no more: it becomes A, X, V and S
        }
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (lane + 64 * t < ne) { sS[ei[t] * LINEAR_Q + ej[t]] = acc[t]; sS[ej[t] * LINEAR_Q + ei[t]] = acc[t]; }
        linear_wave_sync();
        linear_record(C, sS, s_h[m], n1, n2, n_obs, A.mean, sA, sX, sV, s_D[wave], lane, 64, [] { linear_wave_sync(); },
                      A.out + row, A.coef ? A.coef + (size_t)row * (size_t)(2 * p) : nullptr);
    }
}

}  // namespace hpgv
