// hpgv_rows_kernels.h -- the kept rows of a matrix, back to back in source order (hpgv_rows_gather_dev), and the flags that
// select the candidate lines of an association batch (hpgv_assoc_select_text): what clumping keeps of a batch -- the rows with
// p <= p2, about one in a hundred -- without the matrix crossing the bus.
//
//   k_rows_kept_sums / k_head_bases / k_rows_kept_offsets : dst_row[i] = exclusive sum of keep[j] != 0 over j < i, dst_row[n] = K
//                                                           (the heads' three-launch scan, hpgv_text_kernels.h, over ones)
//   k_rows_copy                                           : row i to row dst_row[i] of the destination when kept; index[i] =
//                                                           dst_row[i] or -1; *n_kept = K
//
// The copy moves row_bytes of a kept row and nothing else: whole 16-byte granules where both pitches and both pointers are
// multiples of 16 (then every row of either matrix starts on a granule), the row's last row_bytes % 16 bytes -- or, without that
// alignment, all of them -- as bytes.  No store reaches the bytes between two destination rows or behind the last one.
// Included by hpgv_text_capi.hip only, after hpgv_text_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpgv {

struct KeptOne {
    const uint8_t *__restrict__ keep;
    __device__ __forceinline__ unsigned long long operator()(int i) const { return keep[i] ? 1ull : 0ull; }
};
static __global__ __launch_bounds__(1024) void k_rows_kept_sums(const uint8_t *__restrict__ keep, int n_rows, unsigned long long *__restrict__ block_sum) {
    len_block_sums(KeptOne{keep}, n_rows, block_sum);
}
static __global__ __launch_bounds__(1024) void k_rows_kept_offsets(const uint8_t *__restrict__ keep, int n_rows,
                                                                   const unsigned long long *__restrict__ block_base,
                                                                   unsigned long long *__restrict__ dst_row) {
    len_offsets(KeptOne{keep}, n_rows, block_base, dst_row);
}

// A team of T lanes per row, T the smallest power of two with 16 T >= row_bytes, at most 64: one lane per row up to 16 bytes, a
// wave per row from 1 KB on.  A grid of whole waves strides over the rows, 64 / T of them per wave and turn.
template <bool ALIGNED>
static __global__ __launch_bounds__(256) void k_rows_copy(const uint8_t *__restrict__ src, size_t src_pitch, size_t row_bytes, int n_rows,
                                                          const uint8_t *__restrict__ keep, const unsigned long long *__restrict__ dst_row,
                                                          uint8_t *__restrict__ dst, size_t dst_pitch, int32_t *__restrict__ index,
                                                          int32_t *__restrict__ n_kept) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_kept = (int32_t)dst_row[n_rows];
    int T = 1;
    while (T < 64 && 16ull * (unsigned long long)T < row_bytes) T <<= 1;
    const int lane = (int)(threadIdx.x & 63), per_wave = 64 / T, r = lane & (T - 1);
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (blockDim.x >> 6) * per_wave;
    for (long long i = wave * per_wave + lane / T; i < n_rows; i += stride) {
        const bool kept = keep[i] != 0;
        const unsigned long long to = dst_row[i];
        if (r == 0) index[i] = kept ? (int32_t)to : -1;
        if (!kept) continue;                                        // (the whole team: one row)
        const uint8_t *s = src + (size_t)i * src_pitch;
        uint8_t *d = dst + (size_t)to * dst_pitch;
        const size_t whole = ALIGNED ? row_bytes & ~(size_t)15 : 0;
        if (ALIGNED) {
            const uint4 *si = (const uint4 *)s;
            uint4 *o = (uint4 *)d;
            for (size_t k = (size_t)r; k < whole / 16; k += (size_t)T) o[k] = si[k];
        }
        for (size_t k = whole + (size_t)r; k < row_bytes; k += (size_t)T) d[k] = s[k];
    }
}

// keep[i] of hpgv_assoc_select_text: line i is a record (the tokenizer's status byte 0), no record filter rejected it, and
// p <= p_max -- a NaN p never is, p == p_max is.  p_i lies at p + i * p_stride bytes (the statistics kernels' array, or the fused
// kernel's records)
static __global__ __launch_bounds__(256) void k_select_flags(const int32_t *__restrict__ status, const char *__restrict__ p, size_t p_stride, int n,
                                                             double p_max, uint8_t *__restrict__ keep) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int32_t st = status[i];
    const double pv = *(const double *)(p + (size_t)i * p_stride);
    keep[i] = ((st & 0xFF) == 0 && (st & HPGV_LINE_FILTERED) == 0 && pv <= p_max) ? 1 : 0;
}

}  // namespace hpgv
