// hpgv_assoc_cmh_kernels.h -- stratified association (include/hpgv.h "stratified association"; PLINK's --mh / --bd with --within):
// the 2 x 2 allele table of every (variant, stratum) on the matrix cores (gfx950), then Cochran-Mantel-Haenszel, the Mantel-Haenszel
// odds ratio and Breslow-Day per variant.
//
// Tables.  The stratum image has the label matrix's format (hpgv_assoc_perm_kernels.h): rows of `pitch` bytes in the assoc
// layout's column order, 0 under the pads; row 2k is the 0 / 1 indicator "stratum k and affected", row 2k + 1 "stratum k and
// unaffected".  With the planes (c1, c2) of perm_planes
//     {A1_k, A2_k} = sum_j (c1, c2)(v, j) image[2k][j]        {U1_k, U2_k} = sum_j (c1, c2)(v, j) image[2k + 1][j]
// an i8 product with exact i32 sums, v_mfma_i32_16x16x64_i8.
//
// Tile and lane maps are k_assoc_perm's: four waves, 64 variants per workgroup (16 per wave), a lane's 16 row bytes are one
// fragment over the samples k0 + 16 (l >> 4), the image tile of a k-step staged in LDS (rows 80 bytes apart, two buffers, one
// barrier per k-step) and read 16 bytes per lane from the same sample offset.  The OPERANDS ARE SWAPPED: the image rows are A and
// the genotype rows B, so in C/D col = l & 15 is the wave's variant -- the one whose bytes the lane loaded -- and row =
// (l >> 4) * 4 + reg is the image row.  A lane's four registers of an accumulator are then image rows 4q .. 4q + 3 = strata 2q and
// 2q + 1, both classes: {acc1[0], acc2[0], acc1[1], acc2[1]} IS {A1, A2, U1, U2} of stratum 2q and registers 2, 3 give stratum
// 2q + 1.  No shuffle, two 16-byte stores per lane and image tile.
//
// Forms.  NT in {1, 2, 4, 8} image tiles of 16 rows per pass: the smallest that covers the image in one pass (8, 16, 32, 64
// strata), beyond that NT = 8 and ceil(image rows / 128) passes over blockIdx.y, each reading the genotype matrix once.
// No atomics, no floating point: the tables do not depend on pieces, streams or devices.
#pragma once
#include "../../include/hpgv.h"
#include "hpgv_kernels.h"
#include "hpgv_assoc_perm_kernels.h"

namespace hpgv {

struct CmhArgs {
    const uint8_t *gt;               // assoc layout, rows `pitch` bytes apart, pads 0xFF
    size_t pitch;
    int chunks;                      // pitch / 16
    int n_variants;
    const uint8_t *is_x;             // per variant, may be null
    const uint8_t *image;            // [image_rows x pitch] i8 0 / 1, image_rows = 2 n_strata rounded up to 16
    int image_rows, n_strata;
    int4 *tables;                    // [v * n_strata + k] = {A1_k, A2_k, U1_k, U2_k}
};

template <int NT>
__global__ __launch_bounds__(256) void k_assoc_cmh_tables(const CmhArgs A) {
    constexpr int ROWS = NT * 16;                                          // image rows per pass
    constexpr int CPS = ROWS * 4;                                          // image chunks per k-step
    constexpr int LPT = (CPS + 255) / 256;                                 // ... per thread
    __shared__ uint4 img[2][ROWS * PERM_LDS_ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int v_lane = (int)blockIdx.x * PERM_VT + wave * 16 + col;       // the variant whose bytes this lane loads, and whose tables it stores
    const int r0 = (int)blockIdx.y * ROWS;
    const bool v_ok = v_lane < A.n_variants;
    const bool x = v_ok && A.is_x != nullptr && A.is_x[v_lane] != 0;
    const uint8_t *row = A.gt + (size_t)(v_ok ? v_lane : 0) * A.pitch;
    const int steps = (A.chunks + 3) / 4;

    // the image tile of k-step s: ROWS rows x 4 chunks of 16 bytes; rows past the image and chunks past the pitch are zeros
    auto image_chunk = [&](int s, int i) -> uint4 {
        const int r = i >> 2, c = s * 4 + (i & 3);
        if (r0 + r < A.image_rows && c < A.chunks)
            return *reinterpret_cast<const uint4 *>(A.image + (size_t)(r0 + r) * A.pitch + (size_t)c * 16);
        return make_uint4(0u, 0u, 0u, 0u);
    };
    auto gt_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + kq;
        if (v_ok && c < A.chunks) return load16o<false>(row, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);                             // all missing: contributes nothing
    };

    perm_i32x4 acc1[NT], acc2[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) { acc1[n] = perm_i32x4{0, 0, 0, 0}; acc2[n] = perm_i32x4{0, 0, 0, 0}; }
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
        const int i = tid + k * 256;
        if (i < CPS) img[0][(i >> 2) * PERM_LDS_ROW + (i & 3)] = image_chunk(0, i);
    }
    uint4 g = gt_chunk(0);
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        uint4 gn = make_uint4(~0u, ~0u, ~0u, ~0u), ln[LPT];
        if (more) {
            gn = gt_chunk(s + 1);
#pragma unroll
            for (int k = 0; k < LPT; ++k) { const int i = tid + k * 256; if (i < CPS) ln[k] = image_chunk(s + 1, i); }
        }
        perm_i32x4 b1, b2;
        {
            uint32_t c1, c2;
            perm_planes(g.x, x, c1, c2); b1[0] = (int)c1; b2[0] = (int)c2;
            perm_planes(g.y, x, c1, c2); b1[1] = (int)c1; b2[1] = (int)c2;
            perm_planes(g.z, x, c1, c2); b1[2] = (int)c1; b2[2] = (int)c2;
            perm_planes(g.w, x, c1, c2); b1[3] = (int)c1; b2[3] = (int)c2;
        }
        const uint4 *buf = img[s & 1];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const uint4 q = buf[(n * 16 + col) * PERM_LDS_ROW + kq];
            const perm_i32x4 a = {(int)q.x, (int)q.y, (int)q.z, (int)q.w};
            acc1[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b1, acc1[n], 0, 0, 0);
            acc2[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b2, acc2[n], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < LPT; ++k) { const int i = tid + k * 256; if (i < CPS) img[(s + 1) & 1][(i >> 2) * PERM_LDS_ROW + (i & 3)] = ln[k]; }
        }
        __syncthreads();
        g = gn;
    }

    // ---- epilogue: acc[n][r] belongs to variant v_lane and image row r0 + 16 n + 4 kq + r
    if (!v_ok) return;
    int4 *out = A.tables + (size_t)v_lane * (size_t)A.n_strata;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int k = (r0 + n * 16 + kq * 4) >> 1;
        if (k < A.n_strata) out[k] = make_int4(acc1[n][0], acc2[n][0], acc1[n][1], acc2[n][1]);
        if (k + 1 < A.n_strata) out[k + 1] = make_int4(acc1[n][2], acc2[n][2], acc1[n][3], acc2[n][3]);
    }
}

// ---- the statistics of one variant from its K tables: the definition of include/hpgv.h, shared by the device kernel and
// hpgv_cmh_fit (f64, no contraction).  tables[k] = {A1, A2, U1, U2} = (a, b, c, d)
constexpr double CMH_Z95 = 1.959963984540054;
constexpr double CMH_BD_LINEAR = 1e-12;          // |1 - psi| below this: the fitted count by the linear equation

// A thread reads its variant's tables CMH_BURST at a time, the loads issued back to back: 8 x 16 bytes are one 128-byte line, so a
// line is fetched once -- read one table per loop turn, 64 lanes x 64 lines thrash the L1 between turns and every line comes in
// eight times.  Tables past K are zeros: n = 0 takes part in nothing, so the sums and their order are those of the plain loop
constexpr int CMH_BURST = 8;
__host__ __device__ __forceinline__ void cmh_load_burst(const int4 *tables, int k0, int K, int4 (&tb)[CMH_BURST]) {
#pragma unroll
    for (int j = 0; j < CMH_BURST; ++j) tb[j] = k0 + j < K ? tables[k0 + j] : make_int4(0, 0, 0, 0);
}

// One stratum's share of the CMH sums, shared with the permutation kernel (hpgv_assoc_cmh_perm_kernels.h): false when the stratum
// takes no part (n < 2; E and V are then not written), else E_k and V_k by the header's expressions; the caller adds a, E, V
__host__ __device__ __forceinline__ bool cmh_term(double a, double b, double c, double d, double &E, double &V) {
    const double m1 = a + b, m0 = c + d, n1 = a + c, n0 = b + d, n = m1 + m0;
    if (n < 2.0) return false;
    E = (m1 * n1) / n;
    V = ((m1 * m0) * (n1 * n0)) / ((n * n) * (n - 1.0));
    return true;
}
// ... and the statistic of the three sums: NaN unless sum V > 0
__host__ __device__ __forceinline__ double cmh_chisq(double sa, double sE, double sV) {
    const double diff = sa - sE;
    return sV > 0.0 ? (diff * diff) / sV : __builtin_nan("");
}

__host__ __device__ __forceinline__ hpgv_cmh_result cmh_fit_one(const int4 *tables, int K) {
    hpgv_cmh_result res;
    const double nan = __builtin_nan("");
    double sa = 0.0, sE = 0.0, sV = 0.0, sR = 0.0, sS = 0.0, sPR = 0.0, sPSQR = 0.0, sQS = 0.0;
    int n_cmh = 0;
    for (int k0 = 0; k0 < K; k0 += CMH_BURST) {
    int4 tb[CMH_BURST];
    cmh_load_burst(tables, k0, K, tb);
#pragma unroll
    for (int j = 0; j < CMH_BURST; ++j) {
        const int4 t = tb[j];
        const double a = t.x, b = t.y, c = t.z, d = t.w;
        const double n = (a + b) + (c + d);
        double E, V;
        if (!cmh_term(a, b, c, d, E, V)) continue;
        ++n_cmh;
        sa += a;
        sE += E;
        sV += V;
        const double R = (a * d) / n, S = (b * c) / n, P = (a + d) / n, Q = (b + c) / n;
        sR += R; sS += S;
        sPR += P * R; sPSQR += P * S + Q * R; sQS += Q * S;
    }
    }
    res.n_strata_cmh = n_cmh;
    res.chisq = cmh_chisq(sa, sE, sV);
    res.p = chisq_p_value(res.chisq);
    const bool has_or = sR > 0.0 && sS > 0.0;
    const double psi = has_or ? sR / sS : nan;              // (from here on a NaN psi carries itself through)
    const double var = sPR / (2.0 * (sR * sR)) + sPSQR / (2.0 * (sR * sS)) + sQS / (2.0 * (sS * sS));
    const double se = has_or ? sqrt(var) : nan, l = log(psi);
    res.or_mh = psi;
    res.se = se;
    res.l95 = exp(l - CMH_Z95 * se);
    res.u95 = exp(l + CMH_Z95 * se);

    // Breslow-Day: the strata whose four margins are positive
    int n_bd = 0;
    bool ok = has_or && psi < __builtin_inf();
    double x2 = 0.0;
    for (int k0 = 0; k0 < K; k0 += CMH_BURST) {
    int4 tb[CMH_BURST];
    cmh_load_burst(tables, k0, K, tb);
#pragma unroll
    for (int j = 0; j < CMH_BURST; ++j) {
        const int4 t = tb[j];
        const double a = t.x, b = t.y, c = t.z, d = t.w;
        const double m1 = a + b, m0 = c + d, n1 = a + c, n0 = b + d;
        if (!(m1 > 0.0 && m0 > 0.0 && n1 > 0.0 && n0 > 0.0)) continue;
        ++n_bd;
        if (!ok) continue;
        // (1 - psi) A^2 + qb A - psi m1 n1 = 0: the root in [max(0, n1 - m0), min(m1, n1)] is the "+ sqrt" one.  qb >= 0: as
        // 2 psi m1 n1 / (qb + sqrt(disc)), no cancellation; qb < 0 (only with psi < 1): as (sqrt(disc) - qb) / (2 (1 - psi))
        const double qa = 1.0 - psi, qb = (m0 - n1) + psi * (m1 + n1), pc = psi * (m1 * n1);
        double Ak;
        if (fabs(qa) < CMH_BD_LINEAR) Ak = pc / qb;
        else {
            const double root = sqrt(qb * qb + 4.0 * (qa * pc));
            Ak = qb >= 0.0 ? (2.0 * pc) / (qb + root) : (root - qb) / (2.0 * qa);
        }
        const double c2 = m1 - Ak, c3 = n1 - Ak, c4 = (m0 - n1) + Ak;
        if (!(Ak > 0.0 && c2 > 0.0 && c3 > 0.0 && c4 > 0.0)) { ok = false; continue; }
        const double W = 1.0 / (1.0 / Ak + 1.0 / c2 + 1.0 / c3 + 1.0 / c4);
        const double e = a - Ak;
        x2 += (e * e) / W;
    }
    }
    const bool bd = ok && n_bd >= 2;
    res.n_strata_bd = n_bd;
    res.chisq_bd = bd ? x2 : nan;
    res.p_bd = chisq_p_value_df(res.chisq_bd, bd ? n_bd - 1 : 2);      // (NaN in, NaN out)
    return res;
}

static __global__ __launch_bounds__(256) void k_assoc_cmh_stats(const int4 *__restrict__ tables, int n_variants, int n_strata, hpgv_cmh_result *__restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_variants) return;
    out[v] = cmh_fit_one(tables + (size_t)v * (size_t)n_strata, n_strata);
}

}  // namespace hpgv
