// hpgv_epi_wide_kernels.h -- the WIDE form of the listed-combination kernel (hpgv_epi_generic_kernels.h: k_epi_combs), for the
// shapes its packing cannot hold: a (fold, class) group or a class of 65 536 samples or more, and more than EPI_MAX_FOLDS folds
// (up to EPI_WIDE_MAX_FOLDS).  The reference takes both: its counts are plain int (model.c:76-206) and --num-folds is any integer
// (cross_validation.c:247-281).
//
// Same model, same outputs, same work split as k_epi_combs: ONE LANE PER CELL, 256 / 3^order combinations per workgroup, LDS
// atomics for TP / FP / risky bits, one thread per (combination, fold) for the accuracy with the same quotient sequence -- the
// accuracies are bit-equal to the oracle's.  What differs:
//   - affected and unaffected counts are separate 32-bit integers everywhere: no packed halves, no carry between them;
//   - nothing in it is a register array indexed by fold (k_epi_combs keeps uint32_t in[EPI_MAX_FOLDS] per lane), so the fold
//     count is a run-time number bounded only by the host's tables;
//   - the LDS block is dynamic and sized by the launch's fold count: per (combination, fold) TP, FP and as many mask words as
//     the order's cells need (1, 1, 3, 8 words for orders 2 .. 5) -- 12 bytes x 28 x 64 = 21 KB at order 2 and 64 folds.
//
// The form chosen: TWO SWEEPS over the words.  The first gives the two class totals of the lane's cell (and, for the counts-only
// launch, writes every group's count).  The second goes fold by fold: the fold's two in-fold counts, training = total - in-fold,
// the MDR decision at once, the LDS atomics.  Live state per lane: the `order` row pointers, two totals, two in-fold counts.  The
// second read of the rows hits the L1 / L2 (a workgroup reads at most 3 * order * CPW distinct rows of W words; the 200 000-
// sample rows of the bench shape are 25 KB each).  The alternatives -- in-fold counts parked in LDS (64 folds x 2 x 256 lanes x
// 4 bytes = 128 KB: one workgroup per CU) or folds in register banks of 16 (one sweep per bank: five sweeps at 64 folds, and a
// register array again) -- cost more than the second sweep, which is one more pass of loads that mostly hit.
//
// Static figures (hipcc -O3, gfx950; VGPR / SGPR / static LDS / scratch bytes; the dynamic LDS on top), testing | training:
//   order 2   38 / 46 / 0 / 0  |  37 / 48 / 0 / 0        order 4   44 / 44 / 0 / 0  |  44 / 46 / 0 / 0
//   order 3   38 / 46 / 0 / 0  |  37 / 48 / 0 / 0        order 5   50 / 45 / 0 / 0  |  50 / 47 / 0 / 0
#pragma once
#include "hpgv_epi_generic_kernels.h"

namespace hpgv {

// popcount of the AND of the lane's ORDER rows over the words [w_lo, w_hi) (whole 4-word steps: hpgv_epi_set_folds)
template <int ORDER>
__device__ __forceinline__ uint32_t epi_wide_count(const uint32_t *const (&row)[ORDER], uint32_t w_lo, uint32_t w_hi) {
    uint32_t cnt = 0;
    for (uint32_t w = w_lo; w < w_hi; w += 4) {
        uint4 x = *reinterpret_cast<const uint4 *>(row[0] + w);
        #pragma unroll
        for (int s = 1; s < ORDER; ++s) {
            const uint4 y = *reinterpret_cast<const uint4 *>(row[s] + w);
            x.x &= y.x; x.y &= y.y; x.z &= y.z; x.w &= y.w;
        }
        cnt = bcnt_acc(x.x, cnt); cnt = bcnt_acc(x.y, cnt); cnt = bcnt_acc(x.z, cnt); cnt = bcnt_acc(x.w, cnt);
    }
    return cnt;
}

// mask words the cells of an order need
template <int ORDER> struct EpiWideMaskWords { static constexpr int value = (EpiCells<ORDER>::value + 31) / 32; };

// dynamic LDS of a launch: per (combination of the workgroup, fold) TP, FP and the mask words
template <int ORDER>
constexpr size_t epi_wide_lds_bytes(int num_folds) {
    return (size_t)(256 / EpiCells<ORDER>::value) * (size_t)num_folds * (size_t)(2 + EpiWideMaskWords<ORDER>::value) * sizeof(uint32_t);
}

// Arguments and outputs as k_epi_combs; num_folds <= EPI_WIDE_MAX_FOLDS, `folds` and `thr` hold num_folds entries, the launch
// gives epi_wide_lds_bytes<ORDER>(num_folds) bytes of dynamic LDS.
template <int ORDER, bool TRAINING>
__global__ void __launch_bounds__(256) k_epi_combs_wide(const uint32_t *__restrict__ planes, int W, const int32_t *__restrict__ combs, int n_combs,
                                                        const uint32_t *__restrict__ group_w0 /* n_groups + 1 */, int num_folds,
                                                        const EpiFold *__restrict__ folds, int n_affected, int n_unaffected,
                                                        int32_t *__restrict__ counts_out,
                                                        double *__restrict__ acc_out, uint32_t *__restrict__ mask_out,
                                                        const double *__restrict__ thr, EpiCandN *__restrict__ cand,
                                                        unsigned *__restrict__ cand_count, unsigned cand_cap) {
    constexpr int CELLS = EpiCells<ORDER>::value, CPW = 256 / CELLS, MW = EpiWideMaskWords<ORDER>::value;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_wide[];
    const int slots = CPW * num_folds;                               // (combination of the workgroup, fold)
    int *s_tp = reinterpret_cast<int *>(s_wide), *s_fp = s_tp + slots;
    uint32_t *s_mask = s_wide + 2 * slots;                           // [slot][MW]
    const int t = threadIdx.x, lc = t / CELLS, cell = t - lc * CELLS;
    const long comb = (long)blockIdx.x * CPW + lc;
    const bool live = lc < CPW && comb < n_combs;
    if (folds) {
        for (int k = t; k < slots * (2 + MW); k += 256) s_wide[k] = 0;
        __syncthreads();
    }

    // this lane's plane rows: SNP s of the combination, genotype = digit s of the cell (the last SNP varies fastest)
    const uint32_t *row[ORDER];
    {
        int c = cell;
        #pragma unroll
        for (int s = ORDER - 1; s >= 0; --s) {
            const int digit = c % 3; c /= 3;
            const int snp = live ? combs[comb * ORDER + s] : 0;
            row[s] = planes + ((size_t)snp * 3 + (size_t)digit) * (size_t)W;
        }
    }
    // ---- first sweep: the cell's class totals (and the in-fold counts, where the caller wants them) ----
    uint32_t tot_a = 0, tot_u = 0;
    if (live)
        for (int f = 0; f < num_folds; ++f) {
            const uint32_t w_a = group_w0[2 * f], w_u = group_w0[2 * f + 1], w_end = group_w0[2 * f + 2];
            const uint32_t in_a = epi_wide_count<ORDER>(row, w_a, w_u), in_u = epi_wide_count<ORDER>(row, w_u, w_end);
            tot_a += in_a; tot_u += in_u;
            if (counts_out) {
                int32_t *o = counts_out + ((size_t)comb * (size_t)(2 * num_folds) + (size_t)(2 * f)) * CELLS + cell;
                o[0] = (int32_t)in_a; o[CELLS] = (int32_t)in_u;
            }
        }
    if (!folds) return;                                              // (uniform: counts only)

    // ---- second sweep, fold by fold: in-fold counts again, training counts, the high-risk bit, what the cell adds to TP / FP ----
    const float f_na = (float)(unsigned)n_affected, f_nu = (float)(unsigned)n_unaffected;
    const float ratio = f_na / f_nu;
    if (live)
        for (int f = 0; f < num_folds; ++f) {
            if (folds[f].test_a < 0) continue;
            const uint32_t w_a = group_w0[2 * f], w_u = group_w0[2 * f + 1], w_end = group_w0[2 * f + 2];
            const int in_a = (int)epi_wide_count<ORDER>(row, w_a, w_u), in_u = (int)epi_wide_count<ORDER>(row, w_u, w_end);
            const int tr_a = (int)tot_a - in_a, tr_u = (int)tot_u - in_u;
            if (mdr_high_risk<false>(tr_a, tr_u, ratio, f_na, f_nu)) {
                const int add_a = TRAINING ? tr_a : in_a, add_u = TRAINING ? tr_u : in_u;
                const int slot = lc * num_folds + f;
                if (add_a) atomicAdd(&s_tp[slot], add_a);
                if (add_u) atomicAdd(&s_fp[slot], add_u);
                atomicOr(&s_mask[slot * MW + (cell >> 5)], 1u << (cell & 31));
            }
        }
    __syncthreads();
    // ---- one thread per (combination of the workgroup, fold): the confusion matrix's accuracy ----
    for (int k = t; k < slots; k += 256) {
        const int c2 = k / num_folds, f = k - c2 * num_folds;
        const long cb = (long)blockIdx.x * CPW + c2;
        if (cb >= n_combs) continue;
        const EpiFold fo = folds[f];
        if (fo.test_a < 0) continue;
        const int tp = s_tp[k], fp = s_fp[k];
        const int size_a = TRAINING ? n_affected - fo.test_a : fo.test_a, size_u = TRAINING ? n_unaffected - fo.test_u : fo.test_u;
        // evaluate_model BA (model.c:466-467), the quotients formed as in k_epi_pairs (Markstein: the correctly rounded x / y)
        const double TP = (double)tp, TN = (double)(size_u - fp), ya = (double)size_a, yu = (double)size_u;
        double qa = TP * fo.inv_a, qu = TN * fo.inv_u;
        qa = __builtin_fma(__builtin_fma(-qa, ya, TP), fo.inv_a, qa);
        qu = __builtin_fma(__builtin_fma(-qu, yu, TN), fo.inv_u, qu);
        const double acc = (qa + qu) / 2;
        if (acc_out) {
            acc_out[(size_t)cb * (size_t)num_folds + (size_t)f] = acc;
            if (mask_out)
                for (int w = 0; w < EPI_MASK_WORDS; ++w) mask_out[((size_t)cb * (size_t)num_folds + (size_t)f) * EPI_MASK_WORDS + w] = w < MW ? s_mask[k * MW + w] : 0u;
        }
        if (cand && acc >= thr[f]) {                                 // (a NaN accuracy ranks nowhere)
            const unsigned slot = atomicAdd(&cand_count[f], 1u);
            if (slot < cand_cap) {
                EpiCandN e;
                e.accuracy = acc; e.index = (uint32_t)cb; e.pad = 0;
                for (int w = 0; w < EPI_MASK_WORDS; ++w) e.risky[w] = w < MW ? s_mask[k * MW + w] : 0u;
                cand[(size_t)f * cand_cap + slot] = e;
            }
        }
    }
}

}  // namespace hpgv
