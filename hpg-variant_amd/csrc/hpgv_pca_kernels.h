// hpgv_pca_kernels.h -- principal components of a symmetric f64 matrix (include/hpgv.h "PCA"): the kernels of block subspace
// iteration on the GRM.  The first f64 unit of the engine: one block product near the HBM and the FP64 roofs, and four small
// kernels around it.
//
// k_grm_matrix   the n x n buffer of {sq, n} (upper half, diagonal included) as a full f64 matrix, mirrored through LDS so that
//                both halves are written in rows; a pair with n = 0 is 0.0 and counted (one integer add per wave).
// k_pca_apply    Y = A Q for symmetric A (n x n, pitch lda) and Q (n x L, L = 16 or 32) on v_mfma_f64_16x16x4_f64.  One
//                workgroup of four waves owns a PANEL of 64 output rows i and walks all n rows j of A: because A[i][j] = A[j][i]
//                the panel's rows are read as 64 COLUMNS of A, 512 contiguous bytes per row j, two 16-byte loads per lane.  Wave w
//                takes the blocks of 16 rows j with block % 4 == w; the four partial panels are added in wave order through LDS.
//                A lane's first 16-byte load holds columns i0 + 2c, i0 + 2c + 1 (c = lane & 15), its second i0 + 32 + 2c, + 1: the
//                four MFMA row tiles are therefore t -> rows i0 + 32 (t >> 1) + 2 m + (t & 1), m the MFMA's row.  Q is the B
//                operand, one f64 per lane from global memory (Q is n x L x 8 bytes and stays in the L2 / MALL).  C/D map of
//                the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 map.
//                Summation order of Y[i][c]: per wave the blocks in rising order, inside a block the four k-steps in rising
//                order, inside a k-step the MFMA's own order; then ((w0 + w1) + w2) + w3.  It depends on (n, L) only.  No
//                floating-point atomics.  Elements of A at row or column >= n are never read: the last panel and the last
//                block load element by element under a guard.
//                Reading only the upper triangle would halve the traffic; a panel would then add to rows it does not own, which
//                needs a deterministic partial-sum scheme.  Out of scope here.
// k_pca_gram     C = X^T Z (L x L) of two n x L blocks: chunk c of PCA_CHUNK = 256 rows writes partial c (rows in rising
//                order), k_pca_gram_sum adds the partials in chunk order.  The chunking never derives from the device.
// k_pca_rightmul Z = X M, or Z = X M - X' M', for L x L matrices M: one lane per element, k in rising order.
// k_pca_init     the start block from a counter-based generator of (seed, row, column): pca_start_value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpgv {

constexpr int PCA_CHUNK = 256;   // rows of one Gram partial
constexpr int PCA_PANEL = 64;    // output rows of one k_pca_apply workgroup
constexpr int PCA_JBLOCK = 16;   // rows j of one wave's step: four k-steps of the 16x16x4 MFMA

// the start block's element (include/hpgv.h "PCA"): splitmix64's finaliser of a counter made from (seed, row, column), the top
// 53 bits as a fraction, minus one half: uniform in [-0.5, 0.5)
__host__ __device__ inline double pca_start_value(uint64_t seed, uint32_t row, uint32_t col) {
    uint64_t x = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)row * 32ull + (uint64_t)col + 1ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * 0x1p-53 - 0.5;
}

static __global__ __launch_bounds__(256) void k_pca_init(double *__restrict__ Q, int n, int L, uint64_t seed) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= (long long)n * L) return;
    Q[at] = pca_start_value(seed, (uint32_t)(at / L), (uint32_t)(at % L));
}

// grid (T, T) of 32 x 32 tiles, T = ceil(n / 32); a block with tile row above tile column has nothing to do
static __global__ __launch_bounds__(256) void k_grm_matrix(const long long *__restrict__ acc, int n, double scale, double *__restrict__ A, size_t lda,
                                                           unsigned long long *__restrict__ n_empty) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    __shared__ double tile[32][33];
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    unsigned empty = 0;
    for (int r = r0; r < 32; r += 8) {
        const int i = bi * 32 + r, j = bj * 32 + c;
        double v = 0.0;
        if (i < n && j < n && i <= j) {
            const long long sq = acc[((size_t)i * n + j) * 2], cnt = acc[((size_t)i * n + j) * 2 + 1];
            if (cnt == 0) empty++;
            else v = ((double)sq * scale) / (double)cnt;
            A[(size_t)i * lda + j] = v;
        }
        tile[r][c] = v;
    }
    for (int o = 32; o > 0; o >>= 1) empty += __shfl_down(empty, o, 64);
    if ((threadIdx.x & 63) == 0 && empty) atomicAdd(n_empty, (unsigned long long)empty);
    __syncthreads();
    for (int r = r0; r < 32; r += 8) {                    // the mirror: row j of A, columns i of the tile
        const int j = bj * 32 + r, i = bi * 32 + c;
        if (j < n && i < j) A[(size_t)j * lda + i] = tile[c][r];
    }
}

typedef double pca_d4 __attribute__((ext_vector_type(4)));

template <int NT>   // NT = L / 16 column tiles
static __global__ __launch_bounds__(256) void k_pca_apply(const double *__restrict__ A, int n, size_t lda, const double *__restrict__ Q, double *__restrict__ Y) {
    constexpr int L = 16 * NT;
    __shared__ double red[4 * NT * 4 * 64];               // one wave's accumulators, lane-contiguous: 8 or 16 KiB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, kq = lane >> 4;
    const int i0 = blockIdx.x * PCA_PANEL;
    const bool whole = i0 + PCA_PANEL <= n;               // (workgroup-uniform)
    pca_d4 acc[4][NT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = pca_d4{0.0, 0.0, 0.0, 0.0};
    const int n_blocks = (n + PCA_JBLOCK - 1) / PCA_JBLOCK;
    for (int b = wave; b < n_blocks; b += 4) {
        const int j0 = b * PCA_JBLOCK;
        double a[4][4], q[4][NT];
        if (whole && j0 + PCA_JBLOCK <= n) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = j0 + 4 * s + kq;
                const double2 lo = *reinterpret_cast<const double2 *>(A + (size_t)j * lda + i0 + 2 * c);
                const double2 hi = *reinterpret_cast<const double2 *>(A + (size_t)j * lda + i0 + 32 + 2 * c);
                a[s][0] = lo.x; a[s][1] = lo.y; a[s][2] = hi.x; a[s][3] = hi.y;
#pragma unroll
                for (int u = 0; u < NT; ++u) q[s][u] = Q[(size_t)j * L + 16 * u + c];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = j0 + 4 * s + kq;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int i = i0 + 32 * (t >> 1) + 2 * c + (t & 1);
                    a[s][t] = (j < n && i < n) ? A[(size_t)j * lda + i] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < NT; ++u) q[s][u] = j < n ? Q[(size_t)j * L + 16 * u + c] : 0.0;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][t], q[s][u], acc[t][u], 0, 0, 0);
    }
    // the four partial panels in wave order: ((w0 + w1) + w2) + w3; wave 3 holds the sums
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double *p = red + ((t * NT + u) * 4 + r) * 64 + lane;
                        if (w > 0) acc[t][u][r] = *p + acc[t][u][r];
                        if (w < 3) *p = acc[t][u][r];
                    }
        }
        if (w < 3) __syncthreads();
    }
    if (wave != 3) return;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 32 * (t >> 1) + 2 * (kq + 4 * r) + (t & 1);
            if (i < n) {
#pragma unroll
                for (int u = 0; u < NT; ++u) Y[(size_t)i * L + 16 * u + c] = acc[t][u][r];
            }
        }
}

#ifdef HPGV_ABLATION
// The form that lost (DESIGN.md "PCA"): the same panels, blocks, wave split and reduction, but lane l of every wave owns row
// i0 + l of the panel and adds a[j][i] * Q[j][c] with v_fma_f64, the Q row wave-uniform (scalar loads).  Its sums differ from
// k_pca_apply's in the last bits (fma, another order inside a block).
template <int L>
static __global__ __launch_bounds__(256) void k_pca_apply_vector(const double *__restrict__ A, int n, size_t lda, const double *__restrict__ Q, double *__restrict__ Y) {
    __shared__ double red[L * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * PCA_PANEL + lane;
    double acc[L];
#pragma unroll
    for (int c = 0; c < L; ++c) acc[c] = 0.0;
    const int n_blocks = (n + PCA_JBLOCK - 1) / PCA_JBLOCK;
    for (int b = wave; b < n_blocks; b += 4) {
        const int j0 = b * PCA_JBLOCK;
        double a[PCA_JBLOCK];
#pragma unroll
        for (int s = 0; s < PCA_JBLOCK; ++s) a[s] = (j0 + s < n && i < n) ? A[(size_t)(j0 + s) * lda + i] : 0.0;
#pragma unroll
        for (int s = 0; s < PCA_JBLOCK; ++s) {
            if (j0 + s >= n) break;                       // (wave-uniform)
            const double *q = Q + (size_t)(j0 + s) * L;
#pragma unroll
            for (int c = 0; c < L; ++c) acc[c] = fma(a[s], q[c], acc[c]);
        }
    }
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int c = 0; c < L; ++c) {
                double *p = red + c * 64 + lane;
                if (w > 0) acc[c] = *p + acc[c];
                if (w < 3) *p = acc[c];
            }
        }
        if (w < 3) __syncthreads();
    }
    if (wave != 3 || i >= n) return;
#pragma unroll
    for (int c = 0; c < L; ++c) Y[(size_t)i * L + c] = acc[c];
}
#endif

// partial c = X[c * 256 .. ][:]^T Z[same rows][:], rows in rising order; sub-chunks of 64 rows pass through LDS
template <int L>
static __global__ __launch_bounds__(256) void k_pca_gram(const double *__restrict__ X, const double *__restrict__ Z, int n, double *__restrict__ partial) {
    constexpr int PER = L * L / 256;                      // outputs per lane: 1 or 4
    __shared__ double sx[64 * L], sz[64 * L];
    const int row0 = blockIdx.x * PCA_CHUNK;
    double sum[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) sum[k] = 0.0;
    for (int sub = 0; sub < PCA_CHUNK; sub += 64) {
        for (int e = threadIdx.x; e < 64 * L; e += 256) {
            const long long row = (long long)row0 + sub + e / L;
            sx[e] = row < n ? X[row * L + e % L] : 0.0;
            sz[e] = row < n ? Z[row * L + e % L] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int o = threadIdx.x + 256 * k, ca = o / L, cb = o % L;
            double s = sum[k];
            for (int r = 0; r < 64; ++r) s = fma(sx[r * L + ca], sz[r * L + cb], s);
            sum[k] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) partial[(size_t)blockIdx.x * L * L + threadIdx.x + 256 * k] = sum[k];
}

static __global__ __launch_bounds__(256) void k_pca_gram_sum(const double *__restrict__ partial, int n_chunks, int LL, double *__restrict__ C) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= LL) return;
    double s = 0.0;
    for (int c = 0; c < n_chunks; ++c) s += partial[(size_t)c * LL + o];
    C[o] = s;
}

// Z = X M (X2 NULL) or Z = X M - X2 M2: one lane per element, 256 / L rows per workgroup, the small matrices in LDS
template <int L>
static __global__ __launch_bounds__(256) void k_pca_rightmul(const double *__restrict__ X, const double *__restrict__ M, const double *__restrict__ X2,
                                                             const double *__restrict__ M2, int n, double *__restrict__ Z) {
    __shared__ double sm[L * L], sm2[L * L];
    for (int e = threadIdx.x; e < L * L; e += 256) { sm[e] = M[e]; sm2[e] = X2 ? M2[e] : 0.0; }
    __syncthreads();
    const long long row = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    const int col = threadIdx.x % L;
    if (row >= n) return;
    double s = 0.0;
    for (int k = 0; k < L; ++k) s = fma(X[row * L + k], sm[k * L + col], s);
    if (X2) {
        double s2 = 0.0;
        for (int k = 0; k < L; ++k) s2 = fma(X2[row * L + k], sm2[k * L + col], s2);
        s -= s2;
    }
    Z[row * L + col] = s;
}

}  // namespace hpgv
