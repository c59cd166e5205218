// hpgv_grm_kernels.h -- the genetic relationship matrix between the COLUMNS (samples) of one genotype matrix as an EXACT integer
// computation on the matrix cores (gfx950): the per-row table of quantised standardised genotypes, and the pair sums.
//
// A GRM weights every row by 1 / (2 p (1 - p)) inside the sum, so no product of 0 / 1 planes gives it.  The standardised
// genotype z_c = (c - 2 p) / sqrt(2 p (1 - p)) of a row is instead quantised, BY DEFINITION (include/hpgv.h "GRM"), to the 16-bit
// fixed point q_c = rint(z_c 2^s), and q = 256 hi + lo is split into two i8 limbs.  For columns i <= j, summed over the used rows
// called in both,
//     HH = sum hi_i hi_j    HL = sum (hi_i lo_j + lo_i hi_j)    LL = sum lo_i lo_j    N = sum v_i v_j
// are five i8 products with exact i32 sums, v_mfma_i32_16x16x64_i8, into four accumulators, and
//     sq = sum q_i q_j = 65536 HH + 256 HL + LL   (int64)        A_ij = (sq 2^-2s) / N
// Integers: the sums do not depend on tile order, row ranges, pieces, streams or devices.
//
// Bounds.  |hi| <= 127 and lo in [-128, 127] (grm_table_value refuses a row with |q| > 127 * 256), so per row |hi_i hi_j| <= 16 129,
// |hi_i lo_j + lo_i hi_j| <= 2 * 127 * 128 = 32 512 and |lo_i lo_j| <= 16 384: an i32 accumulator holds 66 052 rows of the
// largest, and a workgroup's row range is never longer than GRM_MAX_RANGE_ROWS = 32 768 (grm_plan_rows), whatever the shape.
//
// Lookup, then transposition.  The tile, the LDS image, the lane maps and the grid are k_ibs_pairs's (hpgv_ibs_kernels.h): a
// thread loads the same four columns of four consecutive rows.  The class dword of such a load -- 0 / 1 / 2 per valid byte, 3 for a
// missing one -- is four columns of ONE row, and is already a v_perm_b32 selector into that row's 4-byte hi table and 4-byte lo
// table (entry 3 is 0): one perm per plane and dword looks the limbs up, and the three planes hi, lo, v are transposed afterwards
// with ibs_transpose4.  BOTH MFMA operands are read from the same LDS image through the same path at the same k, so the lane-map
// argument of hpgv_ibs_kernels.h carries over: the sums depend neither on how the hardware numbers k inside a lane group nor on
// the order in which v_perm_b32 leaves the four k of a dword.
//
// LDS: 2 buffers x 2 sides x 3 planes x 64 columns x 80 bytes = 60 KiB.  A diagonal tile stages one side, wave w runs the blocks
// n >= w and writes i <= j: the diagonal is part of a GRM.
//
// Epilogue.  ADDS {sq, n} into the caller's n_cols x n_cols records of 16 bytes with relaxed device-scope 64-bit integer atomics,
// for i <= j and n != 0.
#pragma once
#include "hpgv_ibs_kernels.h"

namespace hpgv {

constexpr int GRM_MAX_RANGE_ROWS = 32768;  // rows of one workgroup's range at most: 32 768 * 32 512 < 2^31
constexpr int GRM_MAX_Q = 127 * 256;       // |q| of a used row at most: hi stays inside +-127
constexpr int GRM_MAX_FRAC_BITS = 14;

// The table of one row with class counts n0, n1, n2 (include/hpgv.h "GRM"): hi[c], lo[c] of q_c = rint(z_c 2^frac_bits) for the
// classes c = 0, 1, 2, entry 3 (missing) is 0.  f64 in the header's order (the unit is built with -ffp-contract=off).  Returns
// whether the row is used; the table of an unused row is all zeros.  Whether the row is skipped is the caller's to know
__host__ __device__ inline int grm_table_value(int n0, int n1, int n2, int frac_bits, double min_maf, int8_t hi[4], int8_t lo[4]) {
    for (int c = 0; c < 4; ++c) { hi[c] = 0; lo[c] = 0; }
    if (n0 < 0 || n1 < 0 || n2 < 0 || frac_bits < 0 || frac_bits > GRM_MAX_FRAC_BITS) return 0;
    const long long X = 2ll * n0 + n1, Y = n1 + 2ll * n2, T = X + Y;
    if (!(0 < Y && Y < T)) return 0;
    if (!((double)(X < Y ? X : Y) / (double)T >= min_maf)) return 0;
    const double p = (double)Y / (double)T;
    const double d = sqrt(2.0 * p * (1.0 - p));
    const double scale = (double)(1 << frac_bits);
    int q[3];
    for (int c = 0; c < 3; ++c) {
        const double z = ((double)c - 2.0 * p) / d;
        const double r = rint(z * scale);
        if (!(fabs(r) <= (double)GRM_MAX_Q)) return 0;
        q[c] = (int)r;
    }
    for (int c = 0; c < 3; ++c) {
        const int l = (int)(int8_t)(q[c] & 0xFF);
        lo[c] = (int8_t)l;
        hi[c] = (int8_t)((q[c] - l) / 256);
    }
    return 1;
}

// the value of one pair's sums: (sq 2^-2s) / n, the IEEE result for n = 0
__host__ __device__ inline double grm_value(long long sq, long long n, int frac_bits) {
    return ((double)sq * ldexp(1.0, -2 * frac_bits)) / (double)n;
}

// rows per row range of k_grm_pairs: k_ibs_pairs's plan -- the ranges fill the device about four workgroups deep where the tile
// pairs alone do not, none shorter than IBS_SPLIT_ROWS rows -- with at least as many ranges as the cap of GRM_MAX_RANGE_ROWS asks
// for.  A multiple of 64, at least 64, at most the cap
inline int grm_plan_rows(int n_variants, int n_cols, int n_cus) {
    const long long nv = n_variants > 0 ? n_variants : 0;
    const long long tiles = ((long long)(n_cols > 0 ? n_cols : 1) + IBS_T - 1) / IBS_T, pairs = tiles * (tiles + 1) / 2;
    const long long want = (4ll * (n_cus > 0 ? n_cus : 1) + pairs - 1) / pairs, room = (nv + IBS_SPLIT_ROWS - 1) / IBS_SPLIT_ROWS;
    long long splits = want < room ? (want > 1 ? want : 1) : (room > 1 ? room : 1);
    const long long least = (nv + GRM_MAX_RANGE_ROWS - 1) / GRM_MAX_RANGE_ROWS;
    if (splits < least) splits = least;
    // EQUAL ranges, not ranges of the cap and a rest: the grid deals contiguous runs of (range, pair) items to the XCDs, and a short
    // last range would leave the XCDs that draw it idle (measured: 10 000 x 32 832 as 32 768 + 64 rows took twice the time of one range)
    const long long rows = ((nv + splits - 1) / splits + 63) / 64 * 64;             // <= the cap: the cap is a multiple of 64
    return (int)(rows < 64 ? 64 : rows);
}

// class4 {n0, n1, n2, missing} of every row -> its table record {hi[4], lo[4]} (8 bytes); an unused row gets zeros and
// skip[row] = 1 (a row that comes in skipped is unused whatever its counts); the used rows are counted: by ballot, one relaxed add
// per wave.  One lane per row
static __global__ __launch_bounds__(256) void k_grm_table(const int4 *__restrict__ class4, int n_variants, int frac_bits, double min_maf,
                                                          uint8_t *__restrict__ skip, uint2 *__restrict__ tab, int *__restrict__ n_used) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    bool used = false;
    if (row < n_variants) {
        int8_t hi[4], lo[4];
        const int4 c = class4[row];
        used = skip[row] == 0 && grm_table_value(c.x, c.y, c.z, frac_bits, min_maf, hi, lo) != 0;
        uint32_t h = 0, l = 0;
        if (used) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                h |= (uint32_t)(uint8_t)hi[k] << (8 * k);
                l |= (uint32_t)(uint8_t)lo[k] << (8 * k);
            }
        } else {
            skip[row] = 1;
        }
        tab[row] = make_uint2(h, l);
    }
    const unsigned long long mask = __ballot(used);
    if (n_used != nullptr && mask != 0 && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)mask) - 1))
        __hip_atomic_fetch_add(n_used, (int)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct GrmArgs {
    const uint8_t *gt;               // rows of HPGV8 bytes `pitch` apart
    size_t pitch;
    int n_variants, n_cols;
    const uint8_t *skip;             // per row, may be null
    const uint2 *tab;                // per row {hi[4], lo[4]}
    long long *acc;                  // [(i * n_cols + j) * 2 + k], k = sq, n: added to for i <= j
    long long pairs;                 // tiles (tiles + 1) / 2, tiles = ceil(n_cols / IBS_T)
    int splits, rows_per_split;      // row ranges; rows of each, a multiple of 64, at most GRM_MAX_RANGE_ROWS
    unsigned long long items;        // pairs * splits
    unsigned per_xcd;                // ceil(items / 8)
};

// the planes of one raw dword (four columns of one row) with that row's tables: hi and lo limb of q, valid
__device__ __forceinline__ void grm_planes(uint32_t w, uint2 t, uint32_t &hi, uint32_t &lo, uint32_t &v) {
    uint32_t g;
    perm_planes_trend(w, v, g);
    const uint32_t cls = g | ((v ^ 0x01010101u) * 3u);                     // 0 / 1 / 2, 3 for a missing byte: selector bytes into t
    hi = __builtin_amdgcn_perm(0u, t.x, cls);
    lo = __builtin_amdgcn_perm(0u, t.y, cls);
}

static __global__ __launch_bounds__(256) void k_grm_pairs(const GrmArgs A) {
    __shared__ uint4 img[2][2][3][IBS_T * IBS_LDS_COL];                    // [buffer][side I / J][plane hi, lo, v]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    // workgroup -> (row range, tile pair): "Grid" of hpgv_ibs_kernels.h
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
    const long long k_first = (long long)split * A.rows_per_split;
    if (k_first >= A.n_variants) return;
    const int k_begin = (int)k_first;
    const int k_end = (int)min((long long)A.n_variants, k_first + A.rows_per_split);
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

    // a row that is skipped or past the range loads as 0xFF with a zero table: it adds to no sum
    auto fetch = [&](int s, uint32_t (&ra)[4], uint32_t (&rb)[4], uint2 (&t)[4]) {
        const int kb = k_begin + s * 64 + 4 * rg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kb + r;
            const bool ok = k < k_end && (A.skip == nullptr || A.skip[k] == 0);
            const uint8_t *row = A.gt + (size_t)(ok ? k : 0) * A.pitch;
            t[r] = ok ? A.tab[k] : make_uint2(0u, 0u);
            ra[r] = (ok && ci_ok) ? *reinterpret_cast<const uint32_t *>(row + ci) : ~0u;
            rb[r] = (ok && cj_ok) ? *reinterpret_cast<const uint32_t *>(row + cj) : ~0u;
        }
    };
    auto stage_side = [&](int buf, int side, const uint32_t (&r)[4], const uint2 (&t)[4]) {
        uint32_t hi[4], lo[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) grm_planes(r[k], t[k], hi[k], lo[k], v[k]);
        ibs_transpose4(hi);
        ibs_transpose4(lo);
        ibs_transpose4(v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int at = (4 * cg + c) * (IBS_LDS_COL * 4) + rg;          // in dwords
            reinterpret_cast<uint32_t *>(img[buf][side][0])[at] = hi[c];
            reinterpret_cast<uint32_t *>(img[buf][side][1])[at] = lo[c];
            reinterpret_cast<uint32_t *>(img[buf][side][2])[at] = v[c];
        }
    };
    auto stage = [&](int buf, const uint32_t (&ra)[4], const uint32_t (&rb)[4], const uint2 (&t)[4]) {
        stage_side(buf, 0, ra, t);
        if (!diag) stage_side(buf, 1, rb, t);
    };

    // per block the sums HH, HL, LL, N
    perm_i32x4 acc[IBS_NT][4];
#pragma unroll
    for (int n = 0; n < IBS_NT; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[n][k] = perm_i32x4{0, 0, 0, 0};

    uint32_t ra[4], rb[4];
    uint2 tb[4];
    fetch(0, ra, rb, tb);
    stage(0, ra, rb, tb);
    __syncthreads();

    const int bside = diag ? 0 : 1;
    auto frag = [&](int buf, int side, int plane, int at) -> perm_i32x4 {
        const uint4 q = img[buf][side][plane][at];
        return perm_i32x4{(int)q.x, (int)q.y, (int)q.z, (int)q.w};
    };
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) fetch(s + 1, ra, rb, tb);
        if (any) {
            const int cur = s & 1;
            const int at_a = (wave * 16 + col) * IBS_LDS_COL + kq;
            const perm_i32x4 ah = frag(cur, 0, 0, at_a), al = frag(cur, 0, 1, at_a), av = frag(cur, 0, 2, at_a);
#pragma unroll
            for (int n = 0; n < IBS_NT; ++n) {
                if (!live[n]) continue;
                const int at_b = (n * 16 + col) * IBS_LDS_COL + kq;
                const perm_i32x4 bh = frag(cur, bside, 0, at_b), bl = frag(cur, bside, 1, at_b), bv = frag(cur, bside, 2, at_b);
                acc[n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, acc[n][0], 0, 0, 0);
                acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, acc[n][1], 0, 0, 0);
                acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, acc[n][1], 0, 0, 0);
                acc[n][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, acc[n][2], 0, 0, 0);
                acc[n][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc[n][3], 0, 0, 0);
            }
        }
        if (more) stage((s + 1) & 1, ra, rb, tb);
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
            if (i > j || nn == 0) continue;                                // (no row called in both: both sums are 0)
            const long long sq = 65536ll * acc[n][0][r] + 256ll * acc[n][1][r] + (long long)acc[n][2][r];
            long long *o = A.acc + ((size_t)i * (size_t)A.n_cols + (size_t)j) * 2;
            if (sq) __hip_atomic_fetch_add(o + 0, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(o + 1, (long long)nn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace hpgv
