// hpgv_score_kernels.h -- allele scoring (include/hpgv.h "Score"): per COLUMN (sample) the sum over the rows of weight x ALT
// count, for up to 32 weight columns at once, as an EXACT integer computation on the matrix cores (gfx950): the per-row table of
// quantised weights, and the column sums.
//
// A weight is quantised, BY DEFINITION, to the fixed point q = rint(w 2^s) with |q| <= 2^28, and a used row contributes
// c + qg g to a column on a called byte and c + qm on a missing one (qg, qm, c of the header: flip and mean imputation are folded
// into them).  qg and qm are split into four balanced i8 limbs, and with the planes g (0 / 1 / 2, 0 where missing) and
// m (1 where missing on a row that is not skipped) of the transposed genotypes
//     acc_l[k][j] = sum_rows limb_l(qg_k) g_j + limb_l(qm_k) m_j        sum_k[j] = sum_l acc_l[k][j] 256^l   (int64)
// is two v_mfma_i32_16x16x64_i8 per four scores and k-step of 64 rows: the A operand is 16 rows of (score, limb) x 64 variants,
// the B operand 64 variants x 16 columns.  One row of ones against each plane gives n_alt and the missing calls of a column.
// Integers: the sums do not depend on tile order, row ranges, pieces, streams or devices.
//
// Bounds.  Per row and column only one of g, m is non-zero and |limb g| <= 128 * 2 = 256, so an i32 accumulator holds
// 2^31 / 256 = 2^23 rows; a workgroup's row range is never longer than SCORE_MAX_RANGE_ROWS = 2^22 (score_plan_rows).
//
// The k order of the two operands.  In k_ibs_pairs and k_grm_pairs BOTH operands come out of the same LDS image, so any
// numbering of k inside a lane group cancels.  Here A comes from table memory and B from the transposition, and what must hold is
// this: byte p of the 16 bytes that lane (m, kq) gives as A and byte p of the 16 bytes that lane (n, kq) gives as B belong to the
// SAME variant.  The hardware pairs the operands' k at equal (lane group, byte), whatever it calls that k, so nothing more is needed.
// B: cols_transpose4 leaves the four rows of a column in byte order (row 0 in byte 0: v_perm_b32's selector byte i names the source
// of OUTPUT byte i, and sources 0 .. 3 are the second operand), thread rg = tid >> 4 stores rows 4 rg .. 4 rg + 3 as dword rg of
// the column's 64 k bytes, and lane group kq reads bytes 16 kq .. 16 kq + 15: variant k0 + 16 kq + p at byte p.  A: the table is
// limb-plane-major, tab[(k * 8 + l) * tab_pitch + row], and lane (m, kq) loads the 16 bytes at row k0 + 16 kq of its plane: the
// same variant at byte p.  tests/test_score_gpu.py's one-hot cases pin this.
//
// Latency.  A k-step is short (two MFMAs per four scores), so what a step may not do is wait for its own loads: the genotypes AND the
// table fragments of step s + 1 are loaded before the MFMAs of step s, the skip byte and the genotype dword of a row are loaded
// side by side, and the row ranges are cut eight workgroups per CU deep.  The fragments held a step ahead cost 8 registers per
// score group and plane: 7 waves per SIMD fit at one group, 4 at two, 2 at six, 1 at eight (the compiler's report).
//
// Tile.  A workgroup of four waves owns COLS_T = 64 columns (16 per wave: its B block) and a range of rows; tile geometry, LDS
// image, lane maps, transposition and grid (its unit a tile) are the column tile's (hpgv_cols_kernels.h), one side only: 2 buffers
// x 2 planes x 64 columns x 80 bytes = 20 KiB.  A fragments are plain 16-byte loads of the table, the same for the four waves (L1 / L2).
// C/D: col = l & 15 (the column), row = (l >> 4) * 4 + reg = (score of the group, limb): a lane holds the four limb sums of one
// (score, column) and combines them itself.
//
// Epilogue.  ADDS sum_k[j] into acc[k * acc_pitch + j], n_called into plane n_scores and n_alt into plane n_scores + 1 with
// relaxed device-scope 64-bit integer atomics.  n_called = (rows of the range that are not skipped) - (m-sum of the column).
#pragma once
#include "hpgv_cols_kernels.h"

namespace hpgv {

constexpr int SCORE_MAX = 32;                        // scores per call (HPGV_SCORE_MAX)
constexpr int SCORE_MAX_RANGE_ROWS = 1 << 22;        // rows of one workgroup's range at most: 2^22 * 256 = 2^30
constexpr int SCORE_MAX_FRAC_BITS = 900;             // |frac_bits| at most
constexpr double SCORE_MAX_Q = 268435456.0;          // |q| of a used row at most: 2^28

// the four balanced i8 limbs of v, |v| <= 2^30: v = l[0] + 256 l[1] + 65536 l[2] + 2^24 l[3], the three low ones in [-128, 127]
__host__ __device__ inline void score_limbs(long long v, int8_t l[4]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int b = (int)(int8_t)(v & 0xFF);
        l[i] = (int8_t)b;
        v = (v - b) / 256;
    }
    l[3] = (int8_t)v;
}

// {qg, qm, c} of one weight of a row whose ALT frequency is p (include/hpgv.h "Score"), f64 in the header's order (the unit is
// built with -ffp-contract=off).  Returns whether the weight lets the row be used: finite, |q| <= 2^28
__host__ __device__ inline int score_terms(double w, int s, double p, int flip, int impute, long long *qg, long long *qm, long long *c) {
    *qg = 0; *qm = 0; *c = 0;
    if (!(fabs(w) <= 1.7976931348623157e308)) return 0;                    // NaN, inf
    const double r = rint(ldexp(w, s));
    if (!(fabs(r) <= SCORE_MAX_Q)) return 0;
    const long long q = (long long)r;
    if (!flip) {
        *qg = q;
        *qm = impute ? (long long)rint(ldexp(w * (2.0 * p), s)) : 0;
    } else {
        *qg = -q;
        *c = 2 * q;
        *qm = impute ? (long long)rint(ldexp(w * (2.0 * (1.0 - p)), s)) - 2 * q : -2 * q;
    }
    return 1;
}

// whether a row with these class counts, flags and weights is used, and its ALT frequency
__host__ __device__ inline int score_row_used(int n0, int n1, int n2, const double *w, int n_scores, const int *s, int flags, double *p) {
    *p = 0.0;
    if (n0 < 0 || n1 < 0 || n2 < 0 || (flags & 1)) return 0;
    const long long T = 2ll * ((long long)n0 + n1 + n2);
    if (T <= 0) return 0;
    *p = (double)((long long)n1 + 2ll * n2) / (double)T;
    for (int k = 0; k < n_scores; ++k) {
        long long a, b, c;
        if (!score_terms(w[k], s[k], *p, 0, 0, &a, &b, &c)) return 0;
    }
    return 1;
}

// One row's table (hpgv_score_table): limbs[k * 8 + l], l = 0 .. 3 the limbs of qg_k and 4 .. 7 those of qm_k, and c[k]; zeros
// for an unused row.  Returns whether the row is used
__host__ __device__ inline int score_table_value(int n0, int n1, int n2, const double *w, int n_scores, const int *s, int flags, int impute,
                                                 int8_t *limbs, long long *c) {
    double p;
    const int used = score_row_used(n0, n1, n2, w, n_scores, s, flags, &p);
    for (int k = 0; k < n_scores; ++k) {
        long long qg = 0, qm = 0, ck = 0;
        if (used) score_terms(w[k], s[k], p, (flags >> 1) & 1, impute, &qg, &qm, &ck);
        score_limbs(qg, limbs + k * 8);
        score_limbs(qm, limbs + k * 8 + 4);
        c[k] = ck;
    }
    return used;
}

// ldexp((double)(sum + cnst), -frac_bits)
__host__ __device__ inline double score_value(long long sum, long long cnst, int frac_bits) { return ldexp((double)(sum + cnst), -frac_bits); }

// rows per row range of k_score_cols: the ranges fill the device about eight workgroups deep where the column tiles alone do not
// (200 columns are 4 tiles on 256 CUs), with at least as many ranges as the cap of SCORE_MAX_RANGE_ROWS asks for.  n_scores does
// not enter: a workgroup walks its rows once whatever the number of scores, and more scores only make each step longer
inline int score_plan_rows(int n_variants, int n_cols, int n_scores, int n_cus) {
    (void)n_scores;
    return cols_plan_rows(n_variants, cols_tiles(n_cols), 8, SCORE_MAX_RANGE_ROWS, n_cus);
}

struct ScoreS { int s[SCORE_MAX]; };

// class4 {n0, n1, n2, missing}, the weights and the flag byte of every row -> its limb planes tab[(k * 8 + l) * tab_pitch + row];
// an unused row gets zeros and skip[row] = 1 (a row that comes in skipped is unused whatever else holds); rows from n_variants to
// tab_pitch get zeros.  c_k of the used rows and their number are ADDED to cnst[0 .. n_scores - 1] and cnst[n_scores]: one relaxed
// 64-bit add per wave and non-zero sum.  One lane per row
static __global__ __launch_bounds__(256) void k_score_table(const int4 *__restrict__ class4, int n_variants, const double *__restrict__ w,
                                                            const uint8_t *__restrict__ flags, int n_scores, const ScoreS S, int impute,
                                                            uint8_t *__restrict__ skip, int8_t *__restrict__ tab, size_t tab_pitch,
                                                            long long *__restrict__ cnst) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool used = false;
    double p = 0.0;
    int fl = 0;
    const double *wr = w;
    if (row < (size_t)n_variants) {
        const int4 c = class4[row];
        fl = flags[row];
        wr = w + row * (size_t)n_scores;
        used = skip[row] == 0 && score_row_used(c.x, c.y, c.z, wr, n_scores, S.s, fl, &p) != 0;
        if (!used) skip[row] = 1;
    }
    for (int k = 0; k < n_scores; ++k) {
        long long qg = 0, qm = 0, ck = 0;
        if (used) score_terms(wr[k], S.s[k], p, (fl >> 1) & 1, impute, &qg, &qm, &ck);
        if (row < tab_pitch) {
            int8_t l[8];
            score_limbs(qg, l);
            score_limbs(qm, l + 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) tab[((size_t)k * 8 + i) * tab_pitch + row] = l[i];
        }
        const long long sum = cols_wave_sum_i64(ck);
        if (lane == 0 && sum != 0) __hip_atomic_fetch_add(cnst + k, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long mask = __ballot(used);
    if (lane == 0 && mask != 0) __hip_atomic_fetch_add(cnst + n_scores, (long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct ScoreArgs {
    ColsGrid G;                      // its unit a column tile; a row range has at most SCORE_MAX_RANGE_ROWS rows
    const int8_t *tab;               // limb planes, tab_pitch apart
    size_t tab_pitch;
    int n_scores;
    long long *acc;                  // [k * acc_pitch + col], planes n_scores (n_called) and n_scores + 1 (n_alt) behind the scores
    size_t acc_pitch;
};

// NG: groups of four scores, ceil(n_scores / 4)
template <int NG>
static __global__ __launch_bounds__(256) void k_score_cols(const ScoreArgs A) {
    __shared__ uint4 img[2][2][COLS_T * COLS_LDS_COL];                     // [buffer][plane g, m]
    __shared__ int used_rows;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    const ColsGrid &G = A.G;
    const ColsItem it = cols_item(G);
    if (it.steps == 0) return;                                             // (the whole workgroup)
    const int j0 = (int)it.unit * COLS_T;
    const int k_begin = it.k_begin, k_end = it.k_end, steps = it.steps;
    if (tid == 0) used_rows = 0;

    // what this thread stages: columns 4 cg .. 4 cg + 3 of the tile, rows 4 rg .. 4 rg + 3 of the k-step
    const int cg = tid & 15, rg = tid >> 4;
    const int cj = j0 + 4 * cg;
    const bool cj_ok = cj < G.n_cols;                                      // (cj + 4 <= pitch then: a multiple of 16 >= n_cols)
    const bool live = j0 + wave * 16 < G.n_cols;                           // (wave-uniform)

    // a row that is skipped or past the range loads as 0x00 (g = 0, m = 0) and its table is zeros: it adds to no sum
    int n_ok = 0;
    auto fetch = [&](int s, uint32_t (&r)[4]) {
        const int kb = k_begin + s * 64 + 4 * rg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kb + i;
            const bool in = k < k_end, ok = in && (G.skip == nullptr || G.skip[k] == 0);
            n_ok += ok ? 1 : 0;
            // (the genotypes do not wait for the skip byte: both loads are in flight together)
            const uint32_t w = (in && cj_ok) ? *reinterpret_cast<const uint32_t *>(G.gt + (size_t)k * G.pitch + cj) : 0u;
            r[i] = ok ? w : 0u;
        }
    };
    auto stage = [&](int buf, uint32_t (&r)[4]) {
        cols_transpose4(r);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t v, g;
            perm_planes_trend(r[c], v, g);
            cols_staged(img[buf][0], cg, c, rg) = g;
            cols_staged(img[buf][1], cg, c, rg) = v ^ 0x01010101u;
        }
    };

    // A: lane (m, kq) reads plane (score 4 grp + (m >> 2), limb m & 3) at rows k0 + 16 kq .. + 15; zeros for a score past n_scores
    const int a_score = col >> 2, a_limb = col & 3;
    auto afrag = [&](int grp, int half, int k0) -> perm_i32x4 {
        const int k = grp * 4 + a_score;
        if (k >= A.n_scores) return perm_i32x4{0, 0, 0, 0};
        const uint4 q = *reinterpret_cast<const uint4 *>(A.tab + ((size_t)k * 8 + half * 4 + a_limb) * A.tab_pitch + (size_t)k0 + 16 * kq);
        return perm_i32x4{(int)q.x, (int)q.y, (int)q.z, (int)q.w};
    };
    // the rows of ones: row 0 against g, row 1 against m
    const int one_g = col == 0 ? 0x01010101 : 0, one_m = col == 1 ? 0x01010101 : 0;
    const perm_i32x4 ones_g{one_g, one_g, one_g, one_g}, ones_m{one_m, one_m, one_m, one_m};

    perm_i32x4 acc[NG], cnt = perm_i32x4{0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < NG; ++n) acc[n] = perm_i32x4{0, 0, 0, 0};

    // the table fragments of a k-step are loaded one step ahead, with the genotypes: a step waits for no load of its own
    perm_i32x4 a_cur[NG][2], a_nxt[NG][2];
    auto afetch = [&](int k0, perm_i32x4 (&a)[NG][2]) {                    // (k0 + 63 < tab_pitch: a multiple of 64 >= n_variants)
#pragma unroll
        for (int n = 0; n < NG; ++n) { a[n][0] = afrag(n, 0, k0); a[n][1] = afrag(n, 1, k0); }
    };
    uint32_t r[4];
    fetch(0, r);
    if (live) afetch(k_begin, a_cur);
    stage(0, r);
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) {
            fetch(s + 1, r);
            if (live) afetch(k_begin + (s + 1) * 64, a_nxt);
        }
        if (live) {
            const int cur = s & 1;
            const perm_i32x4 bg = cols_frag(img[cur][0], wave * 16 + col, kq), bm = cols_frag(img[cur][1], wave * 16 + col, kq);
#pragma unroll
            for (int n = 0; n < NG; ++n) {
                acc[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_cur[n][0], bg, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_cur[n][1], bm, acc[n], 0, 0, 0);
            }
            cnt = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones_g, bg, cnt, 0, 0, 0);
            cnt = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones_m, bm, cnt, 0, 0, 0);
        }
        if (more) {
            stage((s + 1) & 1, r);
            if (live) {
#pragma unroll
                for (int n = 0; n < NG; ++n) { a_cur[n][0] = a_nxt[n][0]; a_cur[n][1] = a_nxt[n][1]; }
            }
        }
        __syncthreads();
    }

    // the rows of the range that take part: the threads with cg == 0 saw each row once
    if (cg == 0 && n_ok != 0) atomicAdd(&used_rows, n_ok);
    __syncthreads();
    if (!live) return;

    // ---- epilogue: acc[n][reg] of lane (col, kq) is limb reg of score 4 n + kq in column j
    const int j = j0 + wave * 16 + col;
    if (j >= G.n_cols) return;
#pragma unroll
    for (int n = 0; n < NG; ++n) {
        const int k = n * 4 + kq;
        if (k >= A.n_scores) continue;
        const long long sum = (long long)acc[n][0] + 256ll * acc[n][1] + 65536ll * acc[n][2] + 16777216ll * acc[n][3];
        if (sum) __hip_atomic_fetch_add(A.acc + (size_t)k * A.acc_pitch + j, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (kq == 0) {
        const long long n_called = (long long)used_rows - cnt[1], n_alt = cnt[0];
        if (n_called) __hip_atomic_fetch_add(A.acc + (size_t)A.n_scores * A.acc_pitch + j, n_called, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_alt) __hip_atomic_fetch_add(A.acc + (size_t)(A.n_scores + 1) * A.acc_pitch + j, n_alt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace hpgv
