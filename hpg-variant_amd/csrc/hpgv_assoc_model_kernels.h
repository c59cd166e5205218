// hpgv_assoc_model_kernels.h -- the genotypic model tests of the association path (include/hpgv.h "model tests"; PLINK's
// --model): the genotype-class scan of the resident assoc-layout matrix, and the five statistics of a class table.
//
// Class of an HPGV8 byte: missing when either nibble is 0xF (0xFF and the pads included), else 0 for byte 0x00, 1 when
// exactly one nibble is 0, 2 when both nibbles are alleles other than 0.  Dosage = class.  Chromosome X gets no rule of its
// own -- these are tests on genotypes -- so neither kernel has an is_x parameter.
//
// Scan.  The walk is k_assoc_scan_pipe's: one row per wave, 16 bytes per lane per load, the wave's rows cut into tiles of
// 64 * U chunks, the loads of tile t + 1 issued (assoc_issue_tile, shared) before tile t is counted.  Per dword three
// indicator popcounts on bit 7 of every byte:
//     valid  = ~((isf << 4) | isf)           neither nibble is 0xF
//     homref = ~((ind << 4) | ind)           both nibbles are 0
//     homalt = (ind << 4) & ind & valid      both nibbles are alleles other than 0
// with ind / isf the nibble flags "is not 0" / "is 0xF" on bit 3 of a nibble (model_count_tile): about 14 vector instructions
// per dword, every three-input term one v_bitop3_b32.  A 0xFF byte is in none of the three, so the virtual chunks that fill a
// tile need no bookkeeping; het = valid - homref - homalt and missing = group size - valid at the row end.
//
// The two groups share a register (affected in bits 0..15, unaffected in bits 16..31) as in assoc_row.  A lane adds at most
// 16 per chunk it visits and visits ceil(chunks / 64) chunks of a row, so a half can overflow once 16 * ceil(chunks / 64) >
// 65 535: from 262 081 chunks, a cohort of more than 4 193 280 columns (pad included).  MODEL_MAX_CHUNKS is that bound; the
// launcher refuses wider cohorts (hpgv_set_cohort's own row-length limit is lower still).
#pragma once
#include "hpgv_kernels.h"

namespace hpgv {

constexpr int MODEL_MAX_CHUNKS = 4095 * 64;

struct ModelAcc { uint32_t pvalid, phomref, phomalt; };

template <int U>
__device__ __forceinline__ ModelAcc model_count_tile(const uint4 (&q)[U], int base, int lane, int chunksA, ModelAcc a) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = base + u * 64 + lane;
        const uint32_t sh = (c < chunksA) ? 0u : 16u;
        const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
        uint32_t nv = 0, n0 = 0, n2 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // nibble flags on bit 3, left unmasked: ind = the nibble is not 0 (as nib_nonzero), isf = it is 0xF (the AND of its
            // bits where ind is the OR).  A byte's two flags meet on its bit 7 when the lower one is shifted up by 4, and the
            // byte mask comes in with the same three-input operation
            const uint32_t x = w[k];
            uint32_t ind = x | (x << 1), isf = x & (x << 1);
            ind |= ind << 2;
            isf &= isf << 2;
            const uint32_t valid = ~((isf << 4) | isf) & 0x80808080u;
            nv += __builtin_popcount(valid);
            n0 += __builtin_popcount(~((ind << 4) | ind) & 0x80808080u);
            n2 += __builtin_popcount((ind << 4) & ind & valid);
        }
        a.pvalid += nv << sh;
        a.phomref += n0 << sh;
        a.phomalt += n2 << sh;
    }
    return a;
}

// reduce one row's packed partial sums and store {r0, r1, r2, s0, s1, s2, miss_aff, miss_unaff}
__device__ __forceinline__ void model_row_finish(int lane, int nA, int nU, ModelAcc a, int4 *__restrict__ dst) {
    const int vA = wave_sum((int)(a.pvalid & 0xFFFFu)), vU = wave_sum((int)(a.pvalid >> 16));
    const int r0 = wave_sum((int)(a.phomref & 0xFFFFu)), s0 = wave_sum((int)(a.phomref >> 16));
    const int r2 = wave_sum((int)(a.phomalt & 0xFFFFu)), s2 = wave_sum((int)(a.phomalt >> 16));
    if (lane == 0) {
        dst[0] = make_int4(r0, vA - r0 - r2, r2, s0);
        dst[1] = make_int4(vU - s0 - s2, s2, nA - vA, nU - vU);
    }
}

template <bool NT, int U, int WAVES>
__global__ __launch_bounds__(256, WAVES) void k_assoc_model_scan(const uint8_t *__restrict__ gt, size_t pitch, int n_variants,
                                                                 int chunksA, int chunks, int nA, int nU,
                                                                 int4 *__restrict__ counts8, int vpw) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long v_begin = wave * vpw;
    if (v_begin >= n_variants) return;
    const int rows = (int)((v_begin + vpw <= n_variants) ? vpw : (n_variants - v_begin));
    const int ipr = (chunks + 64 * U - 1) / (64 * U);       // tiles per row
    const int n_tiles = rows * ipr;
    const uint8_t *g0 = gt + (size_t)v_begin * pitch;
    ModelAcc acc = {0u, 0u, 0u};
    auto consume = [&](const uint4 (&q)[U], int t) {
        const int r = t / ipr, it = t - r * ipr;
        acc = model_count_tile<U>(q, it * 64 * U, lane, chunksA, acc);
        if (it == ipr - 1) {
            model_row_finish(lane, nA, nU, acc, counts8 + 2 * (v_begin + r));
            acc.pvalid = acc.phomref = acc.phomalt = 0u;
        }
    };
    uint4 qa[U], qb[U];
    assoc_issue_tile<NT, U>(qa, g0, pitch, 0, ipr, chunks, lane);
    for (int t = 0; t < n_tiles; t += 2) {
        if (t + 1 < n_tiles) assoc_issue_tile<NT, U>(qb, g0, pitch, t + 1, ipr, chunks, lane);
        consume(qa, t);
        if (t + 1 < n_tiles) {
            if (t + 2 < n_tiles) assoc_issue_tile<NT, U>(qa, g0, pitch, t + 2, ipr, chunks, lane);
            consume(qb, t + 1);
        }
    }
}

// ---------------------------------------------------------------------------
// statistics of a class table.  R = r0 + r1 + r2, S = s0 + s1 + s2, N = R + S, n_k = r_k + s_k.
// ---------------------------------------------------------------------------
enum { MODEL_GENO = 0, MODEL_TREND = 1, MODEL_ALLELIC = 2, MODEL_DOM = 3, MODEL_REC = 4 };

// Cochran-Armitage trend test with weights 0, 1, 2: W1 = n1 + 2 n2, W2 = n1 + 4 n2, D = r1 + 2 r2,
//     chi2 = N (N D - R W1)^2 / (R (N - R) (N W2 - W1^2)).
// Operation order, all f64 without contraction:
//     a   = N * D - R * W1
//     num = N * (a * a)
//     den = (R * (N - R)) * (N * W2 - W1 * W1)
//     chi2 = num / den
// The five arguments are integers below 2^23 for any cohort the layout takes (N <= 2.1 M columns, W2 <= 4 N), so N * D,
// R * W1, R * (N - R), N * W2 and W1 * W1 are integers below 2^53: exact, and so are the two subtractions.  den == 0 then
// means exactly that one factor is 0, and each such case makes a == 0 exactly as well:
//     R == 0  => D == 0 (no labelled sample carries dosage)              a = 0 - 0
//     R == N  => D == W1 (every genotyped sample is labelled)            a = N W1 - N W1
//     N W2 == W1^2 (no variance: every genotyped sample has the same dosage k, N == 0 included)
//             => W1 = k N, D = k R                                       a = N k R - R k N
// (these hold for any labelling of the genotyped samples, so for every permuted (R_p, D_p) too).  The result is then
// 0 / 0 = NaN, never +-inf.
__device__ __forceinline__ double trend_chisq_value(int N, int W1, int W2, int R, int D) {
    const double n = N, w1 = W1, w2 = W2, r = R, d = D;
    const double a = n * d - r * w1;
    const double num = n * (a * a);
    const double den = (r * (n - r)) * (n * w2 - w1 * w1);
    return num / den;
}

// df 2: the chi-square survival function is exp(-x / 2)
__device__ __forceinline__ double chisq2_p_value(double x) {
    if (x != x) return x;
    if (x <= 0.0) return 1.0;
    return exp(-x / 2.0);
}

// Pearson chi-square of the 2 x 3 table, every expected value rowtot * coltot / N; an empty margin gives 0 / 0 = NaN
__device__ __forceinline__ double geno_chisq_value(int r0, int r1, int r2, int s0, int s1, int s2) {
    const double R = r0 + r1 + r2, S = s0 + s1 + s2, N = R + S;
    const double n0 = r0 + s0, n1 = r1 + s1, n2 = r2 + s2;
    const double er0 = (R * n0) / N, er1 = (R * n1) / N, er2 = (R * n2) / N;
    const double es0 = (S * n0) / N, es1 = (S * n1) / N, es2 = (S * n2) / N;
    return ((r0 - er0) * (r0 - er0)) / er0 + ((r1 - er1) * (r1 - er1)) / er1 + ((r2 - er2) * (r2 - er2)) / er2 +
           ((s0 - es0) * (s0 - es0)) / es0 + ((s1 - es1) * (s1 - es1)) / es1 + ((s2 - es2) * (s2 - es2)) / es2;
}

// one thread per variant: chisq5[v][t], p5[v][t], t = MODEL_*
static __global__ __launch_bounds__(256) void k_assoc_model_stats(const int4 *__restrict__ counts8, int n,
                                                                  double *__restrict__ chisq5, double *__restrict__ p5) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 lo = counts8[2 * (size_t)i], hi = counts8[2 * (size_t)i + 1];
    const int r0 = lo.x, r1 = lo.y, r2 = lo.z, s0 = lo.w, s1 = hi.x, s2 = hi.y;
    const int R = r0 + r1 + r2, N = R + s0 + s1 + s2, n1 = r1 + s1, n2 = r2 + s2;
    double x[5];
    x[MODEL_GENO] = geno_chisq_value(r0, r1, r2, s0, s1, s2);
    x[MODEL_TREND] = trend_chisq_value(N, n1 + 2 * n2, n1 + 4 * n2, R, r1 + 2 * r2);
    x[MODEL_ALLELIC] = assoc_chisq_value(2 * r0 + r1, r1 + 2 * r2, 2 * s0 + s1, s1 + 2 * s2);
    x[MODEL_DOM] = assoc_chisq_value(r1 + r2, r0, s1 + s2, s0);
    x[MODEL_REC] = assoc_chisq_value(r2, r0 + r1, s2, s0 + s1);
    double *c = chisq5 + 5 * (size_t)i, *p = p5 + 5 * (size_t)i;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        c[t] = x[t];
        p[t] = t == MODEL_GENO ? chisq2_p_value(x[t]) : chisq_p_value(x[t]);
    }
}

}  // namespace hpgv
