// hpgv_ibs_kernels.h -- pairwise identity-by-state counts between the COLUMNS (samples) of one genotype matrix on the matrix
// cores (gfx950), the class counts per row behind the expected values, and the selection of pairs by PI_HAT.
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
// Transposition.  K runs over the ROWS of the matrix, and an operand fragment is 16 consecutive-k bytes of ONE column.  Per
// k-step of 64 rows a thread loads four dwords: the same four columns of four consecutive rows.  Two rounds of v_perm_b32 turn
// them into four dwords that each hold four consecutive k of one column.  The RAW bytes are transposed and the planes formed
// afterwards: the SWAR plane code is bytewise, so it commutes with the permutation, which is then paid once and not per plane.
//
// Lane maps.  A and B: lane l holds column l & 15 of its block and the 16 k values of lane group l >> 4.  BOTH operands are read
// from the LDS image through the same path at the same k -- the A fragment of a column is the very b128 a B fragment of that
// column would be -- so the sums do not depend on how the hardware numbers the k values inside a lane group, nor on the order
// in which v_perm_b32 leaves the four k of a dword.  C/D: col = l & 15 (column j), row = (l >> 4) * 4 + reg (column i).
//
// Tile.  A workgroup of four waves owns IBS_T = 64 columns I (16 per wave) x 64 columns J >= I and a range of rows.  The k-step's
// two 64 x 64 byte blocks are staged in LDS AS PLANES, transposed: 2 sides x 4 planes x 64 columns x 64 bytes, columns 80 bytes
// apart (bank spread of the b128 reads), two buffers, one barrier per k-step: 80 KiB, two workgroups per CU.  Staging raw bytes
// would make each of the four waves form the planes of all 64 J columns again after its reads: 4 times the vector work, and the
// vector ALU, not the matrix pipe, bounds this kernel (DESIGN "IBS").  A diagonal tile stages one side and reads both operands
// from it, computes the blocks on and above the diagonal and writes only i < j.  A block whose columns all lie at or past
// n_cols issues nothing; columns at or past n_cols and rows that are skipped or past the range load as 0xFF.
//
// Grid.  One-dimensional over (row range, tile pair), the pair index fastest.  Workgroups are dealt to the 8 XCDs in turn
// (w % 8) and an XCD's L2 is not shared, so the items are cut into 8 contiguous runs, one per value of w % 8: the workgroups in
// flight on one XCD work on the same row range and on neighbouring tile pairs, which share their J tile.  A matter of speed
// alone (numbering the pairs in super-tiles of 8 x 8 tiles, so that 64 neighbours share 8 + 8 column tiles, measured no
// faster: DESIGN "IBS").  The row ranges exist because few columns give few tiles (200 samples: 10 pairs on 256 CUs).
//
// Epilogue.  ADDS {n, ibs0, ibs1, ibs2} into the caller's n_cols x n_cols records with relaxed device-scope integer atomics:
// row ranges, repeated calls and calls from several streams accumulate into one buffer by construction.
#pragma once
#include "hpgv_assoc_perm_kernels.h"
#include <math.h>

namespace hpgv {

constexpr int IBS_T = 64;            // columns per tile side: 16 per wave on the I side
constexpr int IBS_NT = IBS_T / 16;
constexpr int IBS_LDS_COL = 5;       // uint4 per staged column: 64 k bytes + 16 of padding
constexpr int IBS_SPLIT_ROWS = 256;  // a row range is never shorter than this (but for the last)

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

// the 4 x 4 byte transpose: r[k] holds the bytes of columns c .. c + 3 in row k; afterwards r[c] holds the four rows of column c
__device__ __forceinline__ void ibs_transpose4(uint32_t (&r)[4]) {
    const uint32_t a = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u);   // columns 0, 0, 1, 1 of rows 0 and 1
    const uint32_t b = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);   // columns 2, 2, 3, 3
    const uint32_t c = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u);   // the same of rows 2 and 3
    const uint32_t d = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
    r[0] = __builtin_amdgcn_perm(c, a, 0x05040100u);
    r[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
    r[2] = __builtin_amdgcn_perm(d, b, 0x05040100u);
    r[3] = __builtin_amdgcn_perm(d, b, 0x07060302u);
}

struct IbsArgs {
    const uint8_t *gt;               // rows of HPGV8 bytes `pitch` apart
    size_t pitch;
    int n_variants, n_cols;
    const uint8_t *skip;             // per row, may be null
    int *counts;                     // [(i * n_cols + j) * 4 + k], k = n, ibs0, ibs1, ibs2: added to for i < j
    long long pairs;                 // tiles (tiles + 1) / 2, tiles = ceil(n_cols / IBS_T)
    int splits, rows_per_split;      // row ranges; rows of each, a multiple of 64
    unsigned long long items;        // pairs * splits
    unsigned per_xcd;                // ceil(items / 8)
};

static __global__ __launch_bounds__(256) void k_ibs_pairs(const IbsArgs A) {
    __shared__ uint4 img[2][2][4][IBS_T * IBS_LDS_COL];                    // [buffer][side I / J][plane v, h, m, s]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    // workgroup -> (row range, tile pair), see "Grid" above
    const unsigned seq = blockIdx.x >> 3;
    const unsigned long long item = (unsigned long long)(blockIdx.x & 7u) * A.per_xcd + seq;
    if (seq >= A.per_xcd || item >= A.items) return;                       // (the whole workgroup)
    const int split = (int)(item / (unsigned long long)A.pairs);
    const long long p = (long long)(item % (unsigned long long)A.pairs);
    // p = tj (tj + 1) / 2 + ti with ti <= tj
    long long tj = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((tj + 1) * (tj + 2) / 2 <= p) ++tj;
    while (tj * (tj + 1) / 2 > p) --tj;
    const int ti = (int)(p - tj * (tj + 1) / 2);
    const bool diag = ti == (int)tj;
    const int i0 = ti * IBS_T, j0 = (int)tj * IBS_T;
    const int k_begin = split * A.rows_per_split;
    const int k_end = min(A.n_variants, k_begin + A.rows_per_split);
    if (k_begin >= k_end) return;
    const int steps = (k_end - k_begin + 63) / 64;

    // what this thread stages: columns 4 cg .. 4 cg + 3 of each side, rows 4 rg .. 4 rg + 3 of the k-step
    const int cg = tid & 15, rg = tid >> 4;
    const int ci = i0 + 4 * cg, cj = j0 + 4 * cg;
    const bool ci_ok = ci < A.n_cols, cj_ok = !diag && cj < A.n_cols;      // (ci + 4 <= pitch then: a multiple of 16 >= n_cols)

    // block n of the wave holds the pairs (iw .. iw + 15) x (j0 + 16 n .. j0 + 16 n + 15)
    const int iw = i0 + wave * 16;
    bool live[IBS_NT];
    bool any = false;
#pragma unroll
    for (int n = 0; n < IBS_NT; ++n) {
        live[n] = iw < A.n_cols && j0 + n * 16 < A.n_cols && (!diag || n >= wave);
        any = any || live[n];
    }

    auto fetch = [&](int s, uint32_t (&ra)[4], uint32_t (&rb)[4]) {
        const int kb = k_begin + s * 64 + 4 * rg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kb + r;
            const bool ok = k < k_end && (A.skip == nullptr || A.skip[k] == 0);
            const uint8_t *row = A.gt + (size_t)(ok ? k : 0) * A.pitch;
            ra[r] = (ok && ci_ok) ? *reinterpret_cast<const uint32_t *>(row + ci) : ~0u;
            rb[r] = (ok && cj_ok) ? *reinterpret_cast<const uint32_t *>(row + cj) : ~0u;
        }
    };
    auto stage_side = [&](int buf, int side, uint32_t (&r)[4]) {
        ibs_transpose4(r);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t v, h, m, s;
            ibs_planes(r[c], v, h, m, s);
            const int at = (4 * cg + c) * (IBS_LDS_COL * 4) + rg;          // in dwords
            reinterpret_cast<uint32_t *>(img[buf][side][0])[at] = v;
            reinterpret_cast<uint32_t *>(img[buf][side][1])[at] = h;
            reinterpret_cast<uint32_t *>(img[buf][side][2])[at] = m;
            reinterpret_cast<uint32_t *>(img[buf][side][3])[at] = s;
        }
    };
    auto stage = [&](int buf, uint32_t (&ra)[4], uint32_t (&rb)[4]) {
        stage_side(buf, 0, ra);
        if (!diag) stage_side(buf, 1, rb);
    };

    // per block the sums P1 (s), P2 (m), P3 (h), P4 (v)
    perm_i32x4 acc[IBS_NT][4];
#pragma unroll
    for (int n = 0; n < IBS_NT; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[n][k] = perm_i32x4{0, 0, 0, 0};

    uint32_t ra[4], rb[4];
    fetch(0, ra, rb);
    stage(0, ra, rb);
    __syncthreads();

    const int bside = diag ? 0 : 1;
    auto frag = [&](int buf, int side, int plane, int at) -> perm_i32x4 {
        const uint4 q = img[buf][side][plane][at];
        return perm_i32x4{(int)q.x, (int)q.y, (int)q.z, (int)q.w};
    };
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) fetch(s + 1, ra, rb);
        if (any) {
            const int cur = s & 1;
            const int at_a = (wave * 16 + col) * IBS_LDS_COL + kq;
            const perm_i32x4 av = frag(cur, 0, 0, at_a), ah = frag(cur, 0, 1, at_a), am = frag(cur, 0, 2, at_a), as = frag(cur, 0, 3, at_a);
#pragma unroll
            for (int n = 0; n < IBS_NT; ++n) {
                if (!live[n]) continue;
                const int at_b = (n * 16 + col) * IBS_LDS_COL + kq;
                const perm_i32x4 bv = frag(cur, bside, 0, at_b), bh = frag(cur, bside, 1, at_b);
                const perm_i32x4 bm = frag(cur, bside, 2, at_b), bs = frag(cur, bside, 3, at_b);
                acc[n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(as, bs, acc[n][0], 0, 0, 0);
                acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am, bm, acc[n][1], 0, 0, 0);
                acc[n][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, acc[n][2], 0, 0, 0);
                acc[n][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc[n][3], 0, 0, 0);
            }
        }
        if (more) stage((s + 1) & 1, ra, rb);
        __syncthreads();
    }

    // ---- epilogue: acc[n][k][r] belongs to the pair (i, j) = (iw + 4 kq + r, j0 + 16 n + col)
#pragma unroll
    for (int n = 0; n < IBS_NT; ++n) {
        if (!live[n]) continue;
        const int j = j0 + n * 16 + col;
        if (j >= A.n_cols) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = iw + kq * 4 + r;
            const int nn = acc[n][3][r];
            if (i >= j || nn == 0) continue;                               // (no row called in both: every count is 0)
            const int p1 = acc[n][0][r], p2 = acc[n][1][r], p3 = acc[n][2][r];
            const int ibs0 = (p2 - p1) >> 1, ibs2 = ((p2 + p1) >> 1) + p3, ibs1 = nn - ibs0 - ibs2;
            int *o = A.counts + ((size_t)i * (size_t)A.n_cols + (size_t)j) * 4;
            __hip_atomic_fetch_add(o + 0, nn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ibs0) __hip_atomic_fetch_add(o + 1, ibs0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ibs1) __hip_atomic_fetch_add(o + 2, ibs1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ibs2) __hip_atomic_fetch_add(o + 3, ibs2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// {n0, n1, n2, missing} of every row over the columns below n_cols, one wave per row; a skipped row gets zeros.  No scan of the
// engine yields these for a matrix without a cohort: the stats counters split the calls by allele pair (a "1/2" is in none of
// their four cells) and the model scan's classes are per phenotype group of the assoc layout.
static __global__ __launch_bounds__(256) void k_ibs_class_counts(const uint8_t *__restrict__ gt, size_t pitch, int n_variants, int n_cols,
                                                                 const uint8_t *__restrict__ skip, int4 *__restrict__ class4) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_variants) return;                                         // (the whole wave)
    const bool out = skip != nullptr && skip[row] != 0;
    int n1 = 0, n2 = 0, nv = 0;
    if (!out) {
        const uint8_t *r = gt + (size_t)row * pitch;
        const int chunks = (n_cols + 15) / 16;
        for (int c = lane; c < chunks; c += 64) {
            const uint4 q = load16o<false>(r, (uint32_t)c * 16u);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int left = n_cols - (c * 16 + k * 4);                // columns of this dword below n_cols
                const uint32_t x = left >= 4 ? w[k] : (left <= 0 ? ~0u : (w[k] | (~0u << (8 * left))));
                uint32_t v, g;
                perm_planes_trend(x, v, g);
                nv += __builtin_popcount(v);
                n1 += __builtin_popcount(g & 0x01010101u);
                n2 += __builtin_popcount(g & 0x02020202u);
            }
        }
    }
    nv = wave_sum(nv); n1 = wave_sum(n1); n2 = wave_sum(n2);
    if (lane == 0) class4[row] = out ? make_int4(0, 0, 0, 0) : make_int4(nv - n1 - n2, n1, n2, n_cols - nv);
}

// skip[k] |= is_x[k]: the text form's rule for chromosome X
static __global__ __launch_bounds__(256) void k_ibs_skip_x(uint8_t *__restrict__ skip, const uint8_t *__restrict__ is_x, int n) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k < n && is_x[k] != 0) skip[k] = 1;
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
