// hpgv_ibs_kernels.h -- pairwise identity-by-state counts between the COLUMNS (samples) of one genotype matrix on the matrix
// cores (gfx950), and the selection of pairs by PI_HAT (the class counts per row behind the expected values: hpgv_cols_capi.hip).
//
// For columns i < j with the planes v = valid, h = [g = 1], m = v - h and s = g - 1 on valid bytes (-1, 0, +1 as i8, 0 when
// missing) of their HPGV8 bytes (include/hpgv.h "IBS") the four sums over the rows called in both columns
//     P1 = sum s_i s_j    P2 = sum m_i m_j    P3 = sum h_i h_j    P4 = sum v_i v_j
// are four [samples x variants] x [variants x samples] i8 products with exact i32 sums, v_mfma_i32_16x16x64_i8, and
//     n = P4    ibs0 = (P2 - P1) / 2    ibs2 = (P2 + P1) / 2 + P3    ibs1 = n - ibs0 - ibs2
// (m_i m_j counts the rows where both are homozygous, s_i s_j those of them with the same class minus those with opposite
// classes: the difference is even).  The indicator form (e0 e2 + e2 e0, e0 e0 + e1 e1 + e2 e2, v v) takes six MFMAs per block and
// k-step where this one takes four, from the same number of staged planes: this form was kept.
//
// Tile, LDS image, transposition, lane maps and grid are the column tile's (hpgv_cols_kernels.h): k_ibs_pairs is its pair walk with
// four planes a side -- 2 sides x 4 planes x 64 columns x 80 bytes, two buffers: 80 KiB, two workgroups per CU -- the raw bytes
// transposed before the bytewise plane code, and only i < j written.
//
// Epilogue.  ADDS {n, ibs0, ibs1, ibs2} into the caller's n_cols x n_cols records with relaxed device-scope integer atomics:
// row ranges, repeated calls and calls from several streams accumulate into one buffer by construction.
#pragma once
#include "hpgv_cols_kernels.h"

namespace hpgv {

constexpr long long IBS_MAX_RANGE_ROWS = 2147483584ll;   // 2^31 - 64: a range's rows, rounded up to 64, are an int (its sums: |P| <= rows)

// rows per row range of k_ibs_pairs: about four workgroups per CU deep where the tile pairs alone do not fill the device
inline int ibs_plan_rows(int n_variants, int n_cols, int n_cus) { return cols_plan_rows(n_variants, cols_tile_pairs(n_cols), 4, IBS_MAX_RANGE_ROWS, n_cus); }

// fall(x, k) = x (x - 1) ... (x - k + 1) of include/hpgv.h "IBS": the factors multiplied left to right, fall(x, 0) = 1
__host__ __device__ inline double ibs_fall(double x, int k) {
    double r = 1.0;
    for (int t = 0; t < k; ++t) r = r * (x - (double)t);
    return r;
}

// the five terms {t00, t01, t02, t11, t12} of one row with class counts n0, n1, n2, in the header's operation order; returns
// whether the row is used (T >= 4), zeros when it is not
__host__ __device__ inline int ibs_terms_value(int n0, int n1, int n2, double t[5]) {
    const long long Xi = 2ll * n0 + n1, Yi = n1 + 2ll * n2;
    if (n0 < 0 || n1 < 0 || n2 < 0 || Xi + Yi < 4) { t[0] = t[1] = t[2] = t[3] = t[4] = 0.0; return 0; }
    const double X = (double)Xi, Y = (double)Yi, T = (double)(Xi + Yi);
    auto F = [&](int a, int b) { return (ibs_fall(X, a) * ibs_fall(Y, b)) / ibs_fall(T, a + b); };
    t[0] = 2.0 * F(2, 2);
    t[1] = 4.0 * F(3, 1) + 4.0 * F(1, 3);
    t[2] = (F(4, 0) + F(0, 4)) + 4.0 * F(2, 2);
    t[3] = 2.0 * F(2, 1) + 2.0 * F(1, 2);
    t[4] = ((F(3, 0) + F(0, 3)) + F(2, 1)) + F(1, 2);
    return 1;
}

// {Z0, Z1, Z2, PI_HAT, DST} of one pair's counts with E = {E00, E01, E02, E11, E12}: f64 in this order (the unit is built with
// -ffp-contract=off), S = (double)n:
//     z0 = ibs0 / (E00 S)      z1 = (ibs1 - z0 (E01 S)) / (E11 S)      z2 = (ibs2 - z0 (E02 S) - z1 (E12 S)) / S
//     z0 > 1: (1, 0, 0); then z1 > 1: (0, 1, 0); then z2 > 1: (0, 0, 1)
//     z0 < 0: z1, z2 divided by z1 + z2, z0 = 0; then the same for z1 < 0 over z0 and z2; then for z2 < 0 over z0 and z1
//     PI_HAT = z1 / 2 + z2      DST = (ibs2 + 0.5 ibs1) / S
// Nothing else is special-cased: n = 0 or a zero E give the IEEE NaN or inf that flow through these steps
__host__ __device__ inline void ibs_genome_value(int n, int ibs0, int ibs1, int ibs2, const double *E, double out[5]) {
    const double S = (double)n;
    double z0 = (double)ibs0 / (E[0] * S);
    double z1 = ((double)ibs1 - z0 * (E[1] * S)) / (E[3] * S);
    double z2 = ((double)ibs2 - z0 * (E[2] * S) - z1 * (E[4] * S)) / S;
    if (z0 > 1.0) { z0 = 1.0; z1 = 0.0; z2 = 0.0; }
    if (z1 > 1.0) { z0 = 0.0; z1 = 1.0; z2 = 0.0; }
    if (z2 > 1.0) { z0 = 0.0; z1 = 0.0; z2 = 1.0; }
    if (z0 < 0.0) { const double t = z1 + z2; z1 /= t; z2 /= t; z0 = 0.0; }
    if (z1 < 0.0) { const double t = z0 + z2; z0 /= t; z2 /= t; z1 = 0.0; }
    if (z2 < 0.0) { const double t = z0 + z1; z0 /= t; z1 /= t; z2 = 0.0; }
    out[0] = z0; out[1] = z1; out[2] = z2;
    out[3] = z1 / 2.0 + z2;
    out[4] = ((double)ibs2 + 0.5 * (double)ibs1) / S;
}

// the four planes of 4 packed HPGV8 bytes, one i8 per byte: valid and dosage of perm_planes_trend, then h = [g = 1], m = v - h
// and s = -1 / 0 / +1 for the classes 0 / 1 / 2 of a valid byte
__device__ __forceinline__ void ibs_planes(uint32_t w, uint32_t &v, uint32_t &h, uint32_t &m, uint32_t &s) {
    uint32_t g;
    perm_planes_trend(w, v, g);
    h = g & 0x01010101u;
    m = v ^ h;                                          // (h <= v per byte)
    const uint32_t e2 = (g >> 1) & 0x01010101u;
    s = e2 | ((m ^ e2) * 0xFFu);                        // e0 = m - e2 -> 0xFF per byte, no carry between bytes
}

// k_ibs_pairs's arguments, and its Op of cols_pair_walk: per block the sums P1 (s), P2 (m), P3 (h), P4 (v)
struct IbsArgs {
    ColsGrid G;
    int *counts;                     // [(i * n_cols + j) * 4 + k], k = n, ibs0, ibs1, ibs2: added to for i < j

    static constexpr int NP = 4;     // planes v, h, m, s
    static constexpr bool DIAG = false;
    struct Row {};
    __device__ __forceinline__ Row row(int, bool) const { return Row{}; }
    __device__ __forceinline__ void planes(uint32_t (&r)[4], const Row (&)[4], uint32_t (&pl)[4][4]) const {
        cols_transpose4(r);
#pragma unroll
        for (int c = 0; c < 4; ++c) ibs_planes(r[c], pl[0][c], pl[1][c], pl[2][c], pl[3][c]);
    }
    static __device__ __forceinline__ void mma(const perm_i32x4 (&a)[4], const perm_i32x4 (&b)[4], perm_i32x4 (&acc)[4]) {
        acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[3], b[3], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[2], b[2], acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[1], b[1], acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[0], b[0], acc[3], 0, 0, 0);
    }
    __device__ __forceinline__ void emit(int i, int j, int n_cols, int p1, int p2, int p3, int nn) const {
        if (nn == 0) return;                                               // (no row called in both: every count is 0)
        const int ibs0 = (p2 - p1) >> 1, ibs2 = ((p2 + p1) >> 1) + p3, ibs1 = nn - ibs0 - ibs2;
        int *o = counts + ((size_t)i * (size_t)n_cols + (size_t)j) * 4;
        __hip_atomic_fetch_add(o + 0, nn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ibs0) __hip_atomic_fetch_add(o + 1, ibs0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ibs1) __hip_atomic_fetch_add(o + 2, ibs1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ibs2) __hip_atomic_fetch_add(o + 3, ibs2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

static __global__ __launch_bounds__(256) void k_ibs_pairs(const IbsArgs A) {
    __shared__ uint4 img[2][2][IbsArgs::NP][COLS_T * COLS_LDS_COL];       // [buffer][side I / J][plane]
    cols_pair_walk(A.G, A, img);
}

struct IbsE { double e[5]; };

// The pairs i < j with PI_HAT >= min_pi_hat as records of 32 bytes {i, j, n, ibs0, ibs1, ibs2, pi_hat}: one lane per element of
// the matrix, blocks_per_row workgroups of 256 columns per row i, a workgroup wholly at or below the diagonal returns.  Per wave
// the qualifying lanes are counted by ballot and claim their places with ONE relaxed 64-bit add, as k_ld_edges does; a record
// goes out as two 16-byte stores when its index is below `cap`.  NaN >= x is false: a NaN PI_HAT never qualifies.
static __global__ __launch_bounds__(256) void k_ibs_select(const int4 *__restrict__ counts, int n_cols, int blocks_per_row, const IbsE E, double min_pi_hat,
                                                           uint4 *__restrict__ pairs, unsigned long long cap, unsigned long long *__restrict__ n_pairs) {
    const int lane = threadIdx.x & 63;
    const int i = (int)(blockIdx.x / (unsigned)blocks_per_row);
    const int jb = (int)(blockIdx.x % (unsigned)blocks_per_row) * 256;
    if (jb + 255 <= i) return;                                             // (the whole workgroup)
    const int j = jb + (int)threadIdx.x;
    bool hit = false;
    int4 c = make_int4(0, 0, 0, 0);
    double pi_hat = 0.0;
    if (j > i && j < n_cols) {
        c = counts[(size_t)i * (size_t)n_cols + (size_t)j];
        double out[5];
        ibs_genome_value(c.x, c.y, c.z, c.w, E.e, out);
        pi_hat = out[3];
        hit = pi_hat >= min_pi_hat;
    }
    const unsigned long long mask = __ballot(hit);
    if (mask == 0) return;                                                 // (the whole wave)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
    unsigned long long base = 0;
    if (lane == leader)
        base = __hip_atomic_fetch_add(n_pairs, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)base, leader);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(base >> 32), leader);
    const unsigned long long rank = (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    const unsigned long long at = (((unsigned long long)hi << 32) | lo) + rank;
    if (hit && at < cap) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(pi_hat);
        pairs[2 * at] = make_uint4((unsigned)i, (unsigned)j, (unsigned)c.x, (unsigned)c.y);
        pairs[2 * at + 1] = make_uint4((unsigned)c.z, (unsigned)c.w, (unsigned)bits, (unsigned)(bits >> 32));
    }
}

}  // namespace hpgv
