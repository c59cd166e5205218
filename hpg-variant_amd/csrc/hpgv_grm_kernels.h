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
// Lookup, then transposition.  Tile, LDS image, lane maps and grid are the column tile's (hpgv_cols_kernels.h), k_grm_pairs is its
// pair walk: a thread loads the same four columns of four consecutive rows.  The class dword of such a load -- 0 / 1 / 2 per valid
// byte, 3 for a missing one -- is four columns of ONE row, and is already a v_perm_b32 selector into that row's 4-byte hi table and
// 4-byte lo table (entry 3 is 0): one perm per plane and dword looks the limbs up, and the three planes hi, lo, v are transposed
// afterwards with cols_transpose4.
//
// LDS: 2 buffers x 2 sides x 3 planes x 64 columns x 80 bytes = 60 KiB.  The pairs i == j are written: the diagonal is part of a GRM.
//
// Epilogue.  ADDS {sq, n} into the caller's n_cols x n_cols records of 16 bytes with relaxed device-scope 64-bit integer atomics,
// for i <= j and n != 0.
#pragma once
#include "hpgv_cols_kernels.h"

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

// rows per row range of k_grm_pairs: k_ibs_pairs's depth, and at least as many ranges as the cap of GRM_MAX_RANGE_ROWS asks for
inline int grm_plan_rows(int n_variants, int n_cols, int n_cus) { return cols_plan_rows(n_variants, cols_tile_pairs(n_cols), 4, GRM_MAX_RANGE_ROWS, n_cus); }

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

// the planes of one raw dword (four columns of one row) with that row's tables: hi and lo limb of q, valid
__device__ __forceinline__ void grm_planes(uint32_t w, uint2 t, uint32_t &hi, uint32_t &lo, uint32_t &v) {
    uint32_t g;
    perm_planes_trend(w, v, g);
    const uint32_t cls = g | ((v ^ 0x01010101u) * 3u);                     // 0 / 1 / 2, 3 for a missing byte: selector bytes into t
    hi = __builtin_amdgcn_perm(0u, t.x, cls);
    lo = __builtin_amdgcn_perm(0u, t.y, cls);
}

// k_grm_pairs's arguments, and its Op of cols_pair_walk: per block the sums HH, HL, LL, N.  A row range has at most
// GRM_MAX_RANGE_ROWS rows
struct GrmArgs {
    ColsGrid G;
    const uint2 *tab;                // per row {hi[4], lo[4]}
    long long *acc;                  // [(i * n_cols + j) * 2 + k], k = sq, n: added to for i <= j

    static constexpr int NP = 3;     // planes hi, lo, v
    static constexpr bool DIAG = true;
    typedef uint2 Row;               // a row that is skipped or past the range loads as 0xFF with a zero table: it adds to no sum
    __device__ __forceinline__ Row row(int k, bool ok) const { return ok ? tab[k] : make_uint2(0u, 0u); }
    __device__ __forceinline__ void planes(const uint32_t (&r)[4], const Row (&t)[4], uint32_t (&pl)[3][4]) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) grm_planes(r[k], t[k], pl[0][k], pl[1][k], pl[2][k]);
        cols_transpose4(pl[0]);
        cols_transpose4(pl[1]);
        cols_transpose4(pl[2]);
    }
    static __device__ __forceinline__ void mma(const perm_i32x4 (&a)[3], const perm_i32x4 (&b)[3], perm_i32x4 (&acc)[4]) {
        acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[0], b[0], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[0], b[1], acc[1], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[1], b[0], acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[1], b[1], acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[2], b[2], acc[3], 0, 0, 0);
    }
    __device__ __forceinline__ void emit(int i, int j, int n_cols, int hh, int hl, int ll, int nn) const {
        if (nn == 0) return;                                               // (no row called in both: both sums are 0)
        const long long sq = 65536ll * hh + 256ll * hl + (long long)ll;
        long long *o = acc + ((size_t)i * (size_t)n_cols + (size_t)j) * 2;
        if (sq) __hip_atomic_fetch_add(o + 0, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(o + 1, (long long)nn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

static __global__ __launch_bounds__(256) void k_grm_pairs(const GrmArgs A) {
    __shared__ uint4 img[2][2][GrmArgs::NP][COLS_T * COLS_LDS_COL];       // [buffer][side I / J][plane]
    cols_pair_walk(A.G, A, img);
}

}  // namespace hpgv
