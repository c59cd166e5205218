// hpgv_assoc_perm_kernels.h -- max(T) label permutation of the association test on the matrix cores (gfx950).
//
// For a 0/1 labelling y_p of the cohort columns the permuted allele counts of variant v are
//     A1_p(v) = sum_j c1(v, j) * y_p(j)        A2_p(v) = sum_j c2(v, j) * y_p(j)
// with (c1, c2) in 0..2 the contributions of sample j's HPGV8 byte (perm_planes below): a [variants x samples] x
// [samples x permutations] i8 product with exact i32 sums, v_mfma_i32_16x16x64_i8.  The 16 bytes of a genotype row a lane
// loads are one A fragment (16 consecutive samples of one variant); the label matrix holds one row per permutation in
// the same column order and pitch, so the 16 bytes a lane takes of it are one B fragment over the SAME 16 samples.
//
// Lane maps.  A and B: lane l holds row / column l & 15 and the 16 k values of lane group l >> 4 -- both operands are
// loaded from the same sample offset k0 + 16 (l >> 4), byte for byte, so the sum does not depend on how the hardware
// numbers the k values inside a lane group.  C/D: col = l & 15 (permutation), row = (l >> 4) * 4 + reg (variant).
//
// Tile.  A workgroup of four waves owns PERM_VT = 64 variants (16 per wave) and PERM_PT = 128 permutations.  Per k-step
// of 64 samples a wave loads its 16 x 64 genotype bytes from memory ONCE, turns them into the two i8 planes in registers
// and runs 2 x PERM_PT / 16 MFMAs against the k-step's label tile, which the workgroup stages in LDS (128 rows x 64 bytes,
// rows 80 bytes apart, two buffers: one barrier per k-step).  A launch therefore reads the genotype matrix
// ceil(n_perms / 128) times (the workgroups of one variant tile, blockIdx.y = 0 .. passes - 1); the label matrix (a few
// MB) is read by every variant tile and stays in L2.
//
// Epilogue.  Per (variant, permutation) the chi-square of the permuted table by assoc_chisq_value -- the device function
// of k_assoc_chisq (f64, -ffp-contract=off) -- compared with the observed one.  Counts of T_p >= T_obs are summed over
// the 16 lanes of a row and added with one atomic per (variant, workgroup); the maxima are reduced over the lane groups,
// over the four waves in LDS, and merged with one atomicMax per (permutation, workgroup) on the f64 bit pattern read as
// an unsigned 64-bit integer (the values are >= +0 and never NaN, so the integer order is the numeric one).
//
// Forms.  The kernel has a compile-time form: the statistic decides what the two operand planes hold and what the epilogue
// makes of the two sums; tile, lane maps, staging, reductions and atomics are the same code.
//   PERM_ALLELIC  planes (c1, c2) above, sums {A1_p, A2_p}, assoc_chisq_value of the permuted 2 x 2 allele table
//   PERM_TREND    planes (valid, dosage) of perm_planes_trend, sums {R_p, D_p}, trend_chisq_value(N, W1, W2, R_p, D_p)
//                 (hpgv_assoc_model_kernels.h) with N, W1, W2 of the observed class counts: they do not depend on the labels
#pragma once
#include "hpgv_kernels.h"
#include "hpgv_assoc_model_kernels.h"

namespace hpgv {

constexpr int PERM_VT = 64;          // variants per workgroup: 16 per wave
constexpr int PERM_PT = 128;         // permutations per workgroup
constexpr int PERM_NT = PERM_PT / 16;
constexpr int PERM_LDS_ROW = 5;      // uint4 per staged label row: 64 bytes + 16 of padding (bank spread of the b128 reads)

typedef int perm_i32x4 __attribute__((ext_vector_type(4)));

// per-sample contributions of 4 packed HPGV8 bytes, one i8 per byte: summed over the affected columns they give
// {A1, A2} of k_assoc_scan, over the unaffected ones {U1, U2}
//   autosome: c1 = nibbles equal to 0, c2 = nibbles that are neither 0 nor 0xF     (0xFF: 0, 0)
//   chr X   : c1 = 1 for a byte 0x00, c2 = 1 for a byte whose nibbles are both neither 0 nor 0xF
__device__ __forceinline__ void perm_planes(uint32_t w, bool x, uint32_t &c1, uint32_t &c2) {
    const uint32_t nz = nib_nonzero(w);
    const uint32_t z = ~nz & 0x88888888u;              // bit 3 of a nibble: it is 0
    const uint32_t v = nz & nib_not_f(w);              // bit 3 of a nibble: it is an allele other than 0
    const uint32_t a1 = ((z >> 3) & 0x01010101u) + ((z >> 7) & 0x01010101u);
    const uint32_t a2 = ((v >> 3) & 0x01010101u) + ((v >> 7) & 0x01010101u);
    const uint32_t x1 = ((z & (z >> 4)) >> 3) & 0x01010101u;
    const uint32_t x2 = ((v & (v >> 4)) >> 3) & 0x01010101u;
    c1 = x ? x1 : a1;
    c2 = x ? x2 : a2;
}

// the trend form's planes, one i8 per byte: valid = 1 for a byte without a 0xF nibble, dosage = its genotype class (the
// nibbles of a valid byte that are not 0): 0, 1 or 2.  Summed over the labelled columns they give {R_p, D_p}
__device__ __forceinline__ void perm_planes_trend(uint32_t w, uint32_t &valid, uint32_t &dosage) {
    const uint32_t nf = nib_not_f(w);
    const uint32_t vb = nf & (nf >> 4) & 0x08080808u;  // bit 3 of a byte: both nibbles are called
    const uint32_t nz = nib_nonzero(w) & (vb | (vb << 4));
    valid = vb >> 3;
    dosage = ((nz >> 3) & 0x01010101u) + ((nz >> 7) & 0x01010101u);
}

enum { PERM_ALLELIC = 0, PERM_TREND = 1 };

struct PermArgs {
    const uint8_t *gt;               // assoc layout, rows `pitch` bytes apart, pads 0xFF
    size_t pitch;
    int chunks;                      // pitch / 16
    int n_variants;
    const uint8_t *is_x;             // per variant, may be null (PERM_TREND: not read)
    const int4 *counts;              // observed {A1, A2, U1, U2} of hpgv_assoc_scan_dev; PERM_TREND: the counts8 of
                                     // hpgv_assoc_model_scan_dev, two int4 per variant
    const uint8_t *labels;           // [label_rows x pitch] i8 0 / 1 in the layout's column order, 0 under the pads
    int n_perms, label_rows;
    const uint8_t *skip;             // per variant, may be null: != 0 = the row takes no part (n_ge stays 0)
    int *n_ge;                       // [n_variants], zeroed before the launch
    unsigned long long *batch_max;   // [n_perms] f64 bit patterns, zeroed before the launch
    int *perm_counts;                // [(v * n_perms + p) * 2 + k] or null: the two sums of the form
};

template <int FORM>
__global__ __launch_bounds__(256) void k_assoc_perm(const PermArgs A) {
    __shared__ uint4 lbl[2][PERM_PT * PERM_LDS_ROW];
    __shared__ unsigned long long wg_max[PERM_PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int v_lane = (int)blockIdx.x * PERM_VT + wave * 16 + col;       // the variant whose bytes this lane loads
    const int p0 = (int)blockIdx.y * PERM_PT;
    const bool v_ok = v_lane < A.n_variants;
    const bool x = FORM == PERM_ALLELIC && v_ok && A.is_x != nullptr && A.is_x[v_lane] != 0;
    const uint8_t *row = A.gt + (size_t)(v_ok ? v_lane : 0) * A.pitch;
    const int steps = (A.chunks + 3) / 4;

    // the label tile of k-step s: PERM_PT rows x 4 chunks of 16 bytes, two per thread; rows past the matrix and chunks past
    // the pitch are zeros
    auto label_chunk = [&](int s, int i) -> uint4 {
        const int r = i >> 2, c = s * 4 + (i & 3);
        if (p0 + r < A.label_rows && c < A.chunks)
            return *reinterpret_cast<const uint4 *>(A.labels + (size_t)(p0 + r) * A.pitch + (size_t)c * 16);
        return make_uint4(0u, 0u, 0u, 0u);
    };
    auto gt_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + kq;
        if (v_ok && c < A.chunks) return load16o<false>(row, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);                             // all missing: contributes nothing
    };
    constexpr int LPT = PERM_PT * 4 / 256;                                 // label chunks per thread and k-step
    static_assert(PERM_PT * 4 % 256 == 0, "the label tile is staged by 256 threads");

    perm_i32x4 acc1[PERM_NT], acc2[PERM_NT];
#pragma unroll
    for (int n = 0; n < PERM_NT; ++n) { acc1[n] = perm_i32x4{0, 0, 0, 0}; acc2[n] = perm_i32x4{0, 0, 0, 0}; }
    if (tid < PERM_PT) wg_max[tid] = 0ull;
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
        const int i = tid + k * 256;
        lbl[0][(i >> 2) * PERM_LDS_ROW + (i & 3)] = label_chunk(0, i);
    }
    uint4 g = gt_chunk(0);
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        uint4 gn = make_uint4(~0u, ~0u, ~0u, ~0u), ln[LPT];
        if (more) {
            gn = gt_chunk(s + 1);
#pragma unroll
            for (int k = 0; k < LPT; ++k) ln[k] = label_chunk(s + 1, tid + k * 256);
        }
        perm_i32x4 a1, a2;
        {
            uint32_t c1, c2;
            if constexpr (FORM == PERM_TREND) {
                perm_planes_trend(g.x, c1, c2); a1[0] = (int)c1; a2[0] = (int)c2;
                perm_planes_trend(g.y, c1, c2); a1[1] = (int)c1; a2[1] = (int)c2;
                perm_planes_trend(g.z, c1, c2); a1[2] = (int)c1; a2[2] = (int)c2;
                perm_planes_trend(g.w, c1, c2); a1[3] = (int)c1; a2[3] = (int)c2;
            } else {
                perm_planes(g.x, x, c1, c2); a1[0] = (int)c1; a2[0] = (int)c2;
                perm_planes(g.y, x, c1, c2); a1[1] = (int)c1; a2[1] = (int)c2;
                perm_planes(g.z, x, c1, c2); a1[2] = (int)c1; a2[2] = (int)c2;
                perm_planes(g.w, x, c1, c2); a1[3] = (int)c1; a2[3] = (int)c2;
            }
        }
        const uint4 *buf = lbl[s & 1];
#pragma unroll
        for (int n = 0; n < PERM_NT; ++n) {
            const uint4 q = buf[(n * 16 + col) * PERM_LDS_ROW + kq];
            const perm_i32x4 b = {(int)q.x, (int)q.y, (int)q.z, (int)q.w};
            acc1[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc1[n], 0, 0, 0);
            acc2[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, b, acc2[n], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < LPT; ++k) {
                const int i = tid + k * 256;
                lbl[(s + 1) & 1][(i >> 2) * PERM_LDS_ROW + (i & 3)] = ln[k];
            }
        }
        __syncthreads();
        g = gn;
    }

    // ---- epilogue: acc[n][r] belongs to variant vr0 + r and permutation p0 + 16 n + col
    const int vr0 = (int)blockIdx.x * PERM_VT + wave * 16 + kq * 4;
    double pmax[PERM_NT];
#pragma unroll
    for (int n = 0; n < PERM_NT; ++n) pmax[n] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int v = vr0 + r;
        const bool ok = v < A.n_variants && !(A.skip != nullptr && A.skip[v] != 0);
        int4 o = make_int4(0, 0, 0, 0), o2 = o;                            // trend: {r0, r1, r2, s0}, {s1, s2, miss_aff, miss_unaff}
        if constexpr (FORM == PERM_TREND) { if (ok) { o = A.counts[2 * (size_t)v]; o2 = A.counts[2 * (size_t)v + 1]; } }
        else if (ok) o = A.counts[v];
        const int R1 = o.x + o.z, R2 = o.y + o.w;
        // trend: what does not depend on the labels
        const int n1 = o.y + o2.x, n2 = o.z + o2.y, N = o.x + o.w + n1 + n2, W1 = n1 + 2 * n2, W2 = n1 + 4 * n2;
        // NaN for an empty margin (and for a row left out)
        const double t_obs = FORM == PERM_TREND ? trend_chisq_value(N, W1, W2, o.x + o.y + o.z, o.y + 2 * o.z) : assoc_chisq_value(o.x, o.y, o.z, o.w);
        int cnt = 0;
#pragma unroll
        for (int n = 0; n < PERM_NT; ++n) {
            const int p = p0 + n * 16 + col;
            if (ok && p < A.n_perms) {
                const int a = acc1[n][r], c = acc2[n][r];
                if (A.perm_counts != nullptr)
                    *reinterpret_cast<int2 *>(A.perm_counts + ((size_t)v * (size_t)A.n_perms + (size_t)p) * 2) = make_int2(a, c);
                double t;
                if constexpr (FORM == PERM_TREND) t = trend_chisq_value(N, W1, W2, a, c);
                else t = assoc_chisq_value(a, c, R1 - a, R2 - c);
                if (t >= t_obs) ++cnt;                                     // false when either is NaN
                if (t > pmax[n]) pmax[n] = t;                              // a NaN never enters
            }
        }
        // the 16 lanes of a lane group hold the row's 16 permutations of every n
        cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4); cnt += __shfl_xor(cnt, 8);
        if (col == 0 && cnt > 0) atomicAdd(A.n_ge + v, cnt);
    }
#pragma unroll
    for (int n = 0; n < PERM_NT; ++n) {
        double m = pmax[n], o;
        o = __shfl_xor(m, 16); m = o > m ? o : m;
        o = __shfl_xor(m, 32); m = o > m ? o : m;
        if (kq == 0 && m > 0.0) atomicMax(&wg_max[n * 16 + col], (unsigned long long)__double_as_longlong(m));
    }
    __syncthreads();
    if (tid < PERM_PT && p0 + tid < A.n_perms) {
        const unsigned long long m = wg_max[tid];
        if (m != 0ull) atomicMax(A.batch_max + p0 + tid, m);
    }
}

}  // namespace hpgv
