// hpgv_linear_perm_kernels.h -- max(T) permutations of the linear regression's t statistic on the f64 matrix cores (gfx950;
// include/hpgv.h "permutations of the linear statistic").
//
// Under the Freedman-Lane scheme with mean-imputed missing calls the statistic of row v under permutation p needs two sums,
//     Sd = sum_O d E_p        Sv = sum_O E_p
// over the row's observed positions: a [rows x positions] x [positions x permutations] f64 product with two A planes (the dosage and
// the valid plane of the same genotype bytes), v_mfma_f64_16x16x4_f64.  The permutation image has k_linear's feature layout, in
// tiles of 16 columns: [tile][position][16 doubles], positions padded to whole chunks of 64, zeros under pads.  Tile 0 holds
// Q_1 .. Q_C and e (column C), tile 1 + p / 16 holds E_p in column p % 16; ss[0] = ss_0, ss[1 + p] = ss_p.
//
// k_linear_perm_rows: the row pass.  k_linear's tile walk (linear_tile_walk, both planes) of 16 rows against tile 0, the waves'
//   partial tiles added through LDS in wave order, the class counts as integers; then one thread per row: mu, D, whether the row
//   takes part (linperm_row) and T_obs (linperm_t).  Writes {mu, D} per row (D = 0: takes no part) and t_obs.
// k_linear_perm: the permutation pass.  A workgroup of four waves owns LINPERM_VT = 64 rows (16 per wave) and LINPERM_PT = 128
//   permutations (8 image tiles).  A wave walks ALL positions of its 16 rows in ascending chunks of 64: lane (r, kq) loads the 16
//   bytes of row r at chunk * 64 + 16 kq once, turns byte s into the two A operands in registers and runs 2 x 8 MFMAs per step s
//   against the eight image tiles, whose columns it reads from memory as k_linear reads its features (the lanes of one kq: 128
//   contiguous bytes; the four waves of a workgroup read the same lines).  The order of the sum over the positions is the MFMA's
//   and the walk's, the same for every row wherever it lies in a tile or a call: T_p(v) depends on row v only.
//   Epilogue as k_assoc_perm's: accumulator register t of lane (c, kq) belongs to row 4 t + kq and permutation column c; counts of
//   |T_p| >= |T_obs| summed over the 16 lanes of a row, one integer atomicAdd per (row, workgroup); maxima over the rows in a lane,
//   over the lane groups by shuffles, over the waves in LDS, one atomicMax per (permutation, workgroup) on the bit pattern of the
//   non-negative |T|.  No floating-point atomics.
// Registers and LDS: DESIGN.md "Linear regression".
#pragma once
#include "hpgv_linear_kernels.h"

namespace hpgv {

constexpr int LINPERM_VT = 64;           // rows per workgroup: 16 per wave
constexpr int LINPERM_NT = 8;            // image tiles per workgroup
constexpr int LINPERM_PT = 16 * LINPERM_NT;
constexpr double LINPERM_EPS = 1e-12;

/* ---- the definition's two steps, compiled by the kernels and by the host fit ------------------------------------------------- */

// row scalars -> mu and D; false: the row takes no part.  hd[k] = sum_O d Q_k, hv[k] = sum_O Q_k, k < C
__host__ __device__ inline bool linperm_row(int C, int n_obs, int n1, int n2, int df, const double *hd, const double *hv, double *mu_out, double *D_out) {
    *mu_out = 0.0; *D_out = 0.0;
    if (n_obs == 0 || df < 1) return false;
    const double mu = (double)(n1 + 2 * n2) / (double)n_obs;
    const double sw2 = fma(-(double)n_obs * mu, mu, (double)(n1 + 4 * n2));
    if (!(sw2 > 0.0)) return false;
    double D = sw2;
    for (int k = 0; k < C; ++k) { const double g = fma(-mu, hv[k], hd[k]); D = fma(-g, g, D); }
    if (!(D > LINPERM_EPS * sw2)) return false;
    *mu_out = mu; *D_out = D;
    return true;
}

// (u, D, ss, df) -> T: NaN for r2 >= 1 - 1e-12 and for a NaN r2
__host__ __device__ inline double linperm_t(double u, double D, double ss, int df) {
    const double r2 = (u * u) / (D * ss);
    if (!(r2 < 1.0 - LINPERM_EPS)) return __builtin_nan("");
    const double t = sqrt((double)df * r2 / (1.0 - r2));
    return u < 0.0 ? -t : t;
}

struct LinPermArgs {
    const uint8_t *gt; size_t pitch; int n_variants;   // assoc layout
    int n_cohort, n_covar;
    const double *img;                                 // (1 + tiles) x npos x 16 doubles
    size_t npos;                                       // round_up(pitch, 64)
    const double *ss;                                  // 1 + n_perms
    int n_perms, tiles;                                // tiles = ceil(n_perms / 16)
    const uint8_t *skip;                               // per row, may be null: != 0 = the row takes no part
    double2 *rows;                                     // per row {mu, D}; D = 0: the row takes no part
    double *t_obs;
    int *n_ge;                                         // zeroed before the launch
    unsigned long long *batch_max;                     // [n_perms] f64 bit patterns, zeroed before the launch
    double *perm_t;                                    // [v * n_perms + p] or null
};

__global__ __launch_bounds__(256) void k_linear_perm_rows(const LinPermArgs A) {
    __shared__ double s_part[2][4][256];
    __shared__ double s_sum[2][LINEAR_ROWS][LINEAR_Q];
    __shared__ int s_cnt[4][LINEAR_ROWS][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * LINEAR_ROWS;
    lin_d4 acc = {0.0, 0.0, 0.0, 0.0}, accv = acc;
    int c0 = 0, c1 = 0, c2 = 0;
    linear_tile_walk<true>(A.gt, A.pitch, A.n_variants, row0, A.img, wave, lane, acc, accv, c0, c1, c2);
    c0 += __shfl_xor(c0, 16, 64); c1 += __shfl_xor(c1, 16, 64); c2 += __shfl_xor(c2, 16, 64);
    c0 += __shfl_xor(c0, 32, 64); c1 += __shfl_xor(c1, 32, 64); c2 += __shfl_xor(c2, 32, 64);
    if (kq == 0) { s_cnt[wave][r][0] = c0; s_cnt[wave][r][1] = c1; s_cnt[wave][r][2] = c2; }
#pragma unroll
    for (int t = 0; t < 4; ++t) { s_part[0][wave][t * 64 + lane] = acc[t]; s_part[1][wave][t * 64 + lane] = accv[t]; }
    __syncthreads();
    {   // output row m = 4 t + kq, column r of a wave's tile lies at [t * 64 + lane]; the waves in wave order
        const int m = tid >> 4, c = tid & 15, at = (m >> 2) * 64 + (m & 3) * 16 + c;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) s_sum[pl][m][c] = ((s_part[pl][0][at] + s_part[pl][1][at]) + s_part[pl][2][at]) + s_part[pl][3][at];
    }
    __syncthreads();
    if (tid < LINEAR_ROWS && row0 + tid < A.n_variants) {
        const int m = tid, C = A.n_covar, df = A.n_cohort - (C + 2);
        int n0 = 0, n1 = 0, n2 = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { n0 += s_cnt[w][m][0]; n1 += s_cnt[w][m][1]; n2 += s_cnt[w][m][2]; }
        double mu, D, t = __builtin_nan("");
        const bool skipped = A.skip != nullptr && A.skip[row0 + m] != 0;
        if (!linperm_row(C, n0 + n1 + n2, n1, n2, df, s_sum[0][m], s_sum[1][m], &mu, &D) || skipped) mu = D = 0.0;
        else t = linperm_t(fma(-mu, s_sum[1][m][C], s_sum[0][m][C]), D, A.ss[0], df);
        A.rows[row0 + m] = make_double2(mu, D);
        A.t_obs[row0 + m] = t;
    }
}

// (256, 2): two workgroups per CU -- the register bound that lets a second wave per SIMD hide the operand loads (measured)
__global__ __launch_bounds__(256, 2) void k_linear_perm(const LinPermArgs A) {
    __shared__ unsigned long long wg_max[LINPERM_PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, kq = lane >> 4;
    const int v0 = (int)blockIdx.x * LINPERM_VT + wave * 16;
    const int tile0 = (int)blockIdx.y * LINPERM_NT, p0 = tile0 * 16;
    const bool row_ok = v0 + r < A.n_variants;
    const uint8_t *rp = A.gt + (size_t)(row_ok ? v0 + r : 0) * A.pitch;
    if (tid < LINPERM_PT) wg_max[tid] = 0ull;

    // column r of the workgroup's eight tiles; a tile past the image reads the last one (its sums are never used)
    const double *bp[LINPERM_NT];
#pragma unroll
    for (int n = 0; n < LINPERM_NT; ++n) {
        const int tile = tile0 + n < A.tiles ? tile0 + n : A.tiles - 1;
        bp[n] = A.img + (size_t)(1 + tile) * A.npos * LINEAR_Q + r;
    }
    lin_d4 accd[LINPERM_NT], accv[LINPERM_NT];
#pragma unroll
    for (int n = 0; n < LINPERM_NT; ++n) { accd[n] = lin_d4{0.0, 0.0, 0.0, 0.0}; accv[n] = lin_d4{0.0, 0.0, 0.0, 0.0}; }

    for (size_t base = 0; base < A.pitch; base += 64) {
        const size_t pos = base + 16 * (size_t)kq;
        uint4 g = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (row_ok && pos < A.pitch) g = *reinterpret_cast<const uint4 *>(rp + pos);      // (the pitch is a multiple of 16)
        const unsigned w4[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const unsigned cls = linear_class((w4[s >> 2] >> (8 * (s & 3))) & 0xFFu);
            const double d = cls == 3u ? 0.0 : (double)cls, one = cls == 3u ? 0.0 : 1.0;
            const size_t at = (pos + (size_t)s) * LINEAR_Q;                                // (the image is padded to 64 positions)
#pragma unroll
            for (int n = 0; n < LINPERM_NT; ++n) {
                const double b = bp[n][at];
                accd[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(d, b, accd[n], 0, 0, 0);
                accv[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(one, b, accv[n], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: acc[n][t] belongs to row v0 + 4 t + kq and permutation p0 + 16 n + r
    const int df = A.n_cohort - (A.n_covar + 2);
    double pmax[LINPERM_NT];
#pragma unroll
    for (int n = 0; n < LINPERM_NT; ++n) pmax[n] = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int v = v0 + 4 * t + kq;
        double2 row = make_double2(0.0, 0.0);
        double t_obs = 0.0;
        if (v < A.n_variants) { row = A.rows[v]; t_obs = fabs(A.t_obs[v]); }
        const bool ok = row.y > 0.0;
        int cnt = 0;
#pragma unroll
        for (int n = 0; n < LINPERM_NT; ++n) {
            const int p = p0 + n * 16 + r;
            if (v < A.n_variants && p < A.n_perms) {
                double T = __builtin_nan("");
                if (ok) T = linperm_t(fma(-row.x, accv[n][t], accd[n][t]), row.y, A.ss[1 + p], df);
                if (A.perm_t != nullptr) A.perm_t[(size_t)v * (size_t)A.n_perms + (size_t)p] = T;
                const double a = fabs(T);
                if (a >= t_obs) ++cnt;                                     // false when either is NaN
                if (a > pmax[n]) pmax[n] = a;                              // a NaN never enters
            }
        }
        if (!ok) cnt = 0;                                                  // (T is NaN there anyway)
        // the 16 lanes of a lane group hold the row's 16 permutations of every n
        cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4); cnt += __shfl_xor(cnt, 8);
        if (r == 0 && cnt > 0) atomicAdd(A.n_ge + v, cnt);
    }
    __syncthreads();                                                       // wg_max is zeroed
#pragma unroll
    for (int n = 0; n < LINPERM_NT; ++n) {
        double m = pmax[n], o;
        o = __shfl_xor(m, 16); m = o > m ? o : m;
        o = __shfl_xor(m, 32); m = o > m ? o : m;
        if (kq == 0 && m > 0.0) atomicMax(&wg_max[n * 16 + r], (unsigned long long)__double_as_longlong(m));
    }
    __syncthreads();
    if (tid < LINPERM_PT && p0 + tid < A.n_perms) {
        const unsigned long long m = wg_max[tid];
        if (m != 0ull) atomicMax(A.batch_max + p0 + tid, m);
    }
}

// the f64 matrix cores' own rate (hpgv_mfma_f64_probe): every wave runs `steps` rounds of eight independent MFMAs and no memory
// traffic, two waves per SIMD; the sink is written only by a sum that cannot occur, which keeps the chain alive.  (Sixteen
// accumulators and one wave per SIMD measured LESS: 35.8 against 48.8 T flop/s.)
constexpr int LINPERM_PROBE_ACC = 8;
__global__ __launch_bounds__(256) void k_mfma_f64_probe(int steps, double *sink) {
    lin_d4 acc[LINPERM_PROBE_ACC];
#pragma unroll
    for (int n = 0; n < LINPERM_PROBE_ACC; ++n) acc[n] = lin_d4{0.0, 0.0, 0.0, 0.0};
    const double a = 1.0 + 1e-3 * (double)threadIdx.x, b = 1.0 + 1e-6 * (double)blockIdx.x;
    for (int i = 0; i < steps; ++i) {
#pragma unroll
        for (int n = 0; n < LINPERM_PROBE_ACC; ++n) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[n], 0, 0, 0);
    }
    double sum = 0.0;
#pragma unroll
    for (int n = 0; n < LINPERM_PROBE_ACC; ++n) sum += acc[n][0] + acc[n][1] + acc[n][2] + acc[n][3];
    if (sum == -1.0) sink[0] = sum;
}

}  // namespace hpgv
