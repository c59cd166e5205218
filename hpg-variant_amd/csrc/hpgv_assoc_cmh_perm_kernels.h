// hpgv_assoc_cmh_perm_kernels.h -- max(T) label permutation of the stratified association within its strata (include/hpgv.h
// "stratified association", "Permutation within strata"; PLINK's --mh --mperm with --within) on the matrix cores (gfx950).
//
// For a 0/1 labelling y_p of the cohort columns, stratum k of variant v has the permuted counts
//     a_p,k = sum_{j in stratum k} c1(v, j) y_p(j)        b_p,k = sum_{j in stratum k} c2(v, j) y_p(j)
//     c_p,k = (A1_k + U1_k) - a_p,k                       d_p,k = (A2_k + U2_k) - b_p,k
// with (c1, c2) of perm_planes and {A1_k, A2_k, U1_k, U2_k} the observed table k_assoc_cmh_tables wrote: K i8 products with exact
// i32 sums, v_mfma_i32_16x16x64_i8.  T_p(v) is the CMH chi-square of the K permuted tables by cmh_term / cmh_chisq -- the functions
// cmh_fit_one is made of (hpgv_assoc_cmh_kernels.h), f64 without contraction, the strata summed in the order 0 .. K - 1 -- and
// T_obs(v) the same on the observed tables: bit for bit the record's chisq.
//
// Tile and lane maps are k_assoc_perm's: four waves, 64 variants per workgroup (16 per wave), a lane's 16 row bytes are one A
// fragment over the samples k0 + 16 (l >> 4), the label tile of a k-step double-buffered in LDS (rows 80 bytes apart, one barrier
// per k-step) and read 16 bytes per lane from the same sample offset as B.  C/D: col = l & 15 is the permutation, row =
// (l >> 4) * 4 + reg the variant.  CMH_PERM_NT = 4 accumulator tiles per plane, 64 permutations per workgroup: the running sums
// of a lane are 16 integers and 32 doubles beside the 32 accumulator registers, and under __launch_bounds__(256, 2) the kernel
// keeps to 256 registers without scratch, so two workgroups share a CU and one's f64 stratum epilogue overlaps the other's
// products (DESIGN.md has the register counts of this and of the 128-permutation form, which needs a CU to itself).
//
// Stratum loop.  A workgroup walks the strata in ascending order.  The B tile of stratum k is the label chunk AND the stratum's
// membership mask, which is the OR of rows 2k and 2k + 1 of the stratum image of hpgv_set_strata (no second image: the two
// 16-byte loads per staged chunk are the same addresses for every workgroup and stay in L2 / L1).  After the stratum's k-steps a
// lane holds a_p,k and b_p,k of its 4 variants x 4 x 16 permutations; it reads the four observed tables, adds a, E_k and V_k into
// its running sums (sum a an integer, sum E and sum V f64) and zeroes the accumulators.  Where a_p,k + b_p,k equals the observed
// m1_k -- every row without missing calls in the stratum, under labels shuffled within strata -- E_k and V_k are the ones computed
// once per (variant, stratum) from the observed table: cmh_term of the same inputs, so the same bits.
//
// Sparsity.  Only the k-steps that hold a member of stratum k are visited: `step_off` (K + 1) and `step_idx` are a CSR list of
// ascending 64-column k-steps per stratum, built on the host when the strata are set.  A skipped k-step has an all-zero B tile
// and adds nothing to any sum, so the result is exact.  With stratum-contiguous columns the lists hold about pitch / 64 steps
// in all and the launch does about the matrix-core work of hpgv_assoc_perm_dev at the same number of permutations; with fully
// interleaved columns every stratum lists every step and the launch does up to K times that (and reads the genotype matrix K
// times per pass).  The steps of all strata run as ONE pipelined sequence: the tile of the next stratum's first step is staged
// while the last step of this one is multiplied.
//
// Epilogue.  k_assoc_perm's: T_p >= T_obs counted over the 16 lanes of a row, one integer atomic per (variant, workgroup); the
// maxima over lane groups and waves, one atomicMax per (permutation, workgroup) on the f64 bit pattern; the optional store of T_p.
// Integer atomics and a maximum only: pieces, streams and devices give identical bytes.
#pragma once
#include "hpgv_kernels.h"
#include "hpgv_assoc_perm_kernels.h"
#include "hpgv_assoc_cmh_kernels.h"

namespace hpgv {

constexpr int CMH_PERM_NT = 4;       // accumulator tiles of 16 permutations per plane: 64 permutations per workgroup

struct CmhPermArgs {
    const uint8_t *gt;               // assoc layout, rows `pitch` bytes apart, pads 0xFF
    size_t pitch;
    int chunks;                      // pitch / 16
    int n_variants;
    const uint8_t *is_x;             // per variant, may be null
    const int4 *tables;              // [v * n_strata + k] = {A1_k, A2_k, U1_k, U2_k} of k_assoc_cmh_tables
    const uint8_t *image;            // the stratum image: [2 n_strata rounded up to 16 x pitch] i8 0 / 1
    int n_strata;
    const int *step_off;             // [n_strata + 1]: stratum k's k-steps are step_idx[step_off[k] .. step_off[k + 1])
    const int *step_idx;             // ascending per stratum, each < ceil(chunks / 4)
    const uint8_t *labels;           // [label_rows x pitch] i8 0 / 1, 0 under the pads
    int n_perms, label_rows;
    const uint8_t *skip;             // per variant, may be null: != 0 = the row takes no part (n_ge stays 0)
    int *n_ge;                       // [n_variants], zeroed before the launch
    unsigned long long *batch_max;   // [n_perms] f64 bit patterns, zeroed before the launch
    double *perm_chisq;              // [v * n_perms + p] or null
};

template <int NT>
__global__ __launch_bounds__(256, NT <= 4 ? 2 : 1) void k_assoc_cmh_perm(const CmhPermArgs A) {
    constexpr int PT = NT * 16;                                            // permutations per workgroup
    constexpr int LPT = PT * 4 / 256;                                      // label chunks per thread and k-step
    static_assert(PT * 4 % 256 == 0, "the label tile is staged by 256 threads");
    __shared__ uint4 lbl[2][PT * PERM_LDS_ROW];
    __shared__ unsigned long long wg_max[PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int v_lane = (int)blockIdx.x * PERM_VT + wave * 16 + col;       // the variant whose bytes this lane loads
    const int vr0 = (int)blockIdx.x * PERM_VT + wave * 16 + kq * 4;       // the first of the 4 variants whose sums it holds
    const int p0 = (int)blockIdx.y * PT;
    const int K = A.n_strata;
    const bool v_ok = v_lane < A.n_variants;
    const bool x = v_ok && A.is_x != nullptr && A.is_x[v_lane] != 0;
    const uint8_t *row = A.gt + (size_t)(v_ok ? v_lane : 0) * A.pitch;

    // the B chunk i of stratum k's k-step s: label AND (image row 2k OR image row 2k + 1); rows past the label matrix and chunks
    // past the pitch are zeros
    auto label_chunk = [&](int k, int s, int i) -> uint4 {
        const int r = i >> 2, c = s * 4 + (i & 3);
        if (p0 + r < A.label_rows && c < A.chunks) {
            const uint4 y = *reinterpret_cast<const uint4 *>(A.labels + (size_t)(p0 + r) * A.pitch + (size_t)c * 16);
            const uint8_t *m = A.image + (size_t)(2 * k) * A.pitch + (size_t)c * 16;
            const uint4 ma = *reinterpret_cast<const uint4 *>(m), mu = *reinterpret_cast<const uint4 *>(m + A.pitch);
            return make_uint4(y.x & (ma.x | mu.x), y.y & (ma.y | mu.y), y.z & (ma.z | mu.z), y.w & (ma.w | mu.w));
        }
        return make_uint4(0u, 0u, 0u, 0u);
    };
    auto gt_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + kq;
        if (v_ok && c < A.chunks) return load16o<false>(row, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);                             // all missing: contributes nothing
    };

    perm_i32x4 acc1[NT], acc2[NT];
    int sa[NT][4];
    double sE[NT][4], sV[NT][4];
    int oa[4];                                                             // the observed tables' sums, the same way
    double oE[4], oV[4];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        acc1[n] = perm_i32x4{0, 0, 0, 0}; acc2[n] = perm_i32x4{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) { sa[n][r] = 0; sE[n][r] = 0.0; sV[n][r] = 0.0; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { oa[r] = 0; oE[r] = 0.0; oV[r] = 0.0; }
    if (tid < PT) wg_max[tid] = 0ull;

    // ---- the k-steps of all strata as one sequence t = 0 .. total - 1; k is the stratum of step t (strata without steps have
    // no member column, so their tables are zeros and they take part in nothing)
    const int total = A.step_off[K];
    int k = 0;
    while (k < K && A.step_off[k + 1] <= 0) ++k;
    uint4 g = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (total > 0) {
        const int s0 = A.step_idx[0];
#pragma unroll
        for (int q = 0; q < LPT; ++q) {
            const int i = tid + q * 256;
            lbl[0][(i >> 2) * PERM_LDS_ROW + (i & 3)] = label_chunk(k, s0, i);
        }
        g = gt_chunk(s0);
    }
    __syncthreads();

    for (int t = 0; t < total; ++t) {
        const int tn = t + 1, k_end = A.step_off[k + 1];
        const bool more = tn < total;
        int kn = k;
        uint4 gn = make_uint4(~0u, ~0u, ~0u, ~0u), ln[LPT];
        if (more) {
            while (A.step_off[kn + 1] <= tn) ++kn;                         // (tn < total = step_off[K]: ends at kn < K)
            const int sn = A.step_idx[tn];
            gn = gt_chunk(sn);
#pragma unroll
            for (int q = 0; q < LPT; ++q) ln[q] = label_chunk(kn, sn, tid + q * 256);
        }
        perm_i32x4 a1, a2;
        {
            uint32_t c1, c2;
            perm_planes(g.x, x, c1, c2); a1[0] = (int)c1; a2[0] = (int)c2;
            perm_planes(g.y, x, c1, c2); a1[1] = (int)c1; a2[1] = (int)c2;
            perm_planes(g.z, x, c1, c2); a1[2] = (int)c1; a2[2] = (int)c2;
            perm_planes(g.w, x, c1, c2); a1[3] = (int)c1; a2[3] = (int)c2;
        }
        const uint4 *buf = lbl[t & 1];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const uint4 q = buf[(n * 16 + col) * PERM_LDS_ROW + kq];
            const perm_i32x4 b = {(int)q.x, (int)q.y, (int)q.z, (int)q.w};
            acc1[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc1[n], 0, 0, 0);
            acc2[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, b, acc2[n], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < LPT; ++q) {
                const int i = tid + q * 256;
                lbl[tn & 1][(i >> 2) * PERM_LDS_ROW + (i & 3)] = ln[q];
            }
        }
        __syncthreads();
        g = gn;

        if (tn == k_end) {
            // ---- stratum k is complete: acc[n][r] is (a, b) of variant vr0 + r and permutation p0 + 16 n + col
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int v = vr0 + r;
                const int4 o = v < A.n_variants ? A.tables[(size_t)v * (size_t)K + (size_t)k] : make_int4(0, 0, 0, 0);
                const int n1 = o.x + o.z, n0 = o.y + o.w, m1_obs = o.x + o.y;
                double E0, V0;
                const bool part = cmh_term((double)o.x, (double)o.y, (double)o.z, (double)o.w, E0, V0);      // n = n1 + n0 under every labelling
                if (part) { oa[r] += o.x; oE[r] += E0; oV[r] += V0; }
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int a = acc1[n][r], b = acc2[n][r];
                    double E = E0, V = V0;
                    if (a + b != m1_obs) (void)cmh_term((double)a, (double)b, (double)(n1 - a), (double)(n0 - b), E, V);
                    if (part) { sa[n][r] += a; sE[n][r] += E; sV[n][r] += V; }
                }
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) { acc1[n] = perm_i32x4{0, 0, 0, 0}; acc2[n] = perm_i32x4{0, 0, 0, 0}; }
        }
        k = kn;
    }

    // ---- epilogue: the sums of variant vr0 + r and permutation p0 + 16 n + col
    double pmax[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) pmax[n] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int v = vr0 + r;
        const bool ok = v < A.n_variants && !(A.skip != nullptr && A.skip[v] != 0);
        const double t_obs = cmh_chisq((double)oa[r], oE[r], oV[r]);       // NaN unless sum V > 0
        int cnt = 0;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int p = p0 + n * 16 + col;
            if (ok && p < A.n_perms) {
                const double t = cmh_chisq((double)sa[n][r], sE[n][r], sV[n][r]);
                if (A.perm_chisq != nullptr) A.perm_chisq[(size_t)v * (size_t)A.n_perms + (size_t)p] = t;
                if (t >= t_obs) ++cnt;                                     // false when either is NaN
                if (t > pmax[n]) pmax[n] = t;                              // a NaN never enters
            }
        }
        // the 16 lanes of a lane group hold the row's 16 permutations of every n
        cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4); cnt += __shfl_xor(cnt, 8);
        if (col == 0 && cnt > 0) atomicAdd(A.n_ge + v, cnt);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        double m = pmax[n], o;
        o = __shfl_xor(m, 16); m = o > m ? o : m;
        o = __shfl_xor(m, 32); m = o > m ? o : m;
        if (kq == 0 && m > 0.0) atomicMax(&wg_max[n * 16 + col], (unsigned long long)__double_as_longlong(m));
    }
    __syncthreads();
    if (tid < PT && p0 + tid < A.n_perms) {
        const unsigned long long m = wg_max[tid];
        if (m != 0ull) atomicMax(A.batch_max + p0 + tid, m);
    }
}

}  // namespace hpgv
