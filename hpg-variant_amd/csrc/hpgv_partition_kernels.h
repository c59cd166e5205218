// hpgv_partition_kernels.h -- stable partition of variable-length lines (hpgv_lines_partition_dev, hpgv_text_partition):
// every kept line, byte for byte, back to back in line order, then every other line in line order.  What the filter tool
// writes (hpg-var-vcf filter, filter_runner.c:23-260: the .filtered and .rejected files) when the text is on the device.
//
//   k_kept_sums / k_head_bases / k_kept_offsets : kept_off[i] = exclusive sum of the kept line lengths, kept_off[n] = K
//                                                 (the heads' three-launch scan, hpgv_text_kernels.h, over another length)
//   k_part_copy                                 : line i to kept_off[i], or to K + (line_off[i] - line_off[0]) - kept_off[i]
//
// The copy is bound by HBM: every byte is read once and written once.  The interior of a line goes out in 16-byte stores
// aligned on the destination; the partial granules at its two ends are written with byte stores, so that no byte is stored
// by two lines and no store covers a neighbour's bytes.  The source of an interior granule is an unaligned dwordx4 load
// (shipped) or two aligned ones shifted into place with v_alignbyte (option "part_aligned_loads", ablation build); DESIGN.md
// "Partition of lines" has the A/B.
// Included by hpgv_lines_capi.hip only, after hpgv_text_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hpgv {

struct KeptLen {
    const unsigned long long *__restrict__ line_off; const uint8_t *__restrict__ keep;
    __device__ __forceinline__ unsigned long long operator()(int i) const { return keep[i] ? line_off[i + 1] - line_off[i] : 0ull; }
};
static __global__ __launch_bounds__(1024) void k_kept_sums(const unsigned long long *__restrict__ line_off, const uint8_t *__restrict__ keep,
                                                    int n_lines, unsigned long long *__restrict__ block_sum) {
    len_block_sums(KeptLen{line_off, keep}, n_lines, block_sum);
}
static __global__ __launch_bounds__(1024) void k_kept_offsets(const unsigned long long *__restrict__ line_off, const uint8_t *__restrict__ keep,
                                                       int n_lines, const unsigned long long *__restrict__ block_base,
                                                       unsigned long long *__restrict__ kept_off) {
    len_offsets(KeptLen{line_off, keep}, n_lines, block_base, kept_off);
}

typedef unsigned int part_u32x4 __attribute__((ext_vector_type(4)));
typedef part_u32x4 part_u32x4_u __attribute__((aligned(1)));     // the same, at any byte address (global_load_dwordx4 takes it)

// the 16 bytes at p + sh of the 32 bytes x || y (sh in 1..15): dwords q .. q + 4 of the pair, each output dword one alignbyte
__device__ __forceinline__ part_u32x4 part_shift(part_u32x4 x, part_u32x4 y, unsigned sh) {
    const unsigned q = sh >> 2, b = sh & 3;
    const unsigned c0 = q == 0 ? x.x : q == 1 ? x.y : q == 2 ? x.z : x.w;
    const unsigned c1 = q == 0 ? x.y : q == 1 ? x.z : q == 2 ? x.w : y.x;
    const unsigned c2 = q == 0 ? x.z : q == 1 ? x.w : q == 2 ? y.x : y.y;
    const unsigned c3 = q == 0 ? x.w : q == 1 ? y.x : q == 2 ? y.y : y.z;
    const unsigned c4 = q == 0 ? y.x : q == 1 ? y.y : q == 2 ? y.z : y.w;
    part_u32x4 r;
    r.x = __builtin_amdgcn_alignbyte(c1, c0, b);
    r.y = __builtin_amdgcn_alignbyte(c2, c1, b);
    r.z = __builtin_amdgcn_alignbyte(c3, c2, b);
    r.w = __builtin_amdgcn_alignbyte(c4, c3, b);
    return r;
}

// one line, n bytes from src to dst, by a team of T lanes (r = this lane's rank in it)
template <int ALIGNED_LOADS>
__device__ __forceinline__ void part_copy_line(const char *__restrict__ src, char *__restrict__ dst, unsigned long long n, int r, int T) {
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + n;
    const uintptr_t a0 = (d0 + 15) & ~(uintptr_t)15, a1 = d1 & ~(uintptr_t)15;
    if (a0 >= a1) {                                                 // no whole granule of the destination: bytes
        for (unsigned long long k = (unsigned long long)r; k < n; k += (unsigned)T) dst[k] = src[k];
        return;
    }
    const unsigned long long head = a0 - d0, tail = d1 - a1;        // both < 16
    for (unsigned long long k = (unsigned long long)r; k < head; k += (unsigned)T) dst[k] = src[k];
    for (unsigned long long k = (unsigned long long)r; k < tail; k += (unsigned)T) dst[n - tail + k] = src[n - tail + k];
    const char *s = src + head;                                     // the source of the first whole destination granule
    part_u32x4 *o = (part_u32x4 *)(dst + head);                     // (pointer arithmetic on dst, not on an integer: global stores)
    const unsigned long long g = (a1 - a0) >> 4;
    const unsigned sh = (unsigned)((uintptr_t)s & 15);
    if (sh == 0) {
        const part_u32x4 *si = (const part_u32x4 *)s;
        for (unsigned long long k = (unsigned long long)r; k < g; k += (unsigned)T) o[k] = si[k];
    } else if (ALIGNED_LOADS) {
        // granules k and k + 1 of the source both hold bytes of the line (s + 16 k .. s + 16 k + 15 all lie in it): no load
        // reaches a granule the line does not touch
        const part_u32x4 *si = (const part_u32x4 *)(s - sh);
        for (unsigned long long k = (unsigned long long)r; k < g; k += (unsigned)T) o[k] = part_shift(si[k], si[k + 1], sh);
    } else {
        const part_u32x4_u *su = (const part_u32x4_u *)s;
        for (unsigned long long k = (unsigned long long)r; k < g; k += (unsigned)T) o[k] = su[k];
    }
}

// Lanes per line from the mean line length (the length, not an option): the smallest power of two T with 64 T >= mean, at most
// 64 -- one lane per line up to 64 bytes (sites-only text, a few granules each), a wave per line from 2 KB on (thousands of
// samples).  A grid of whole waves strides over the lines, 64 / T of them per wave and turn.
template <int ALIGNED_LOADS>
__global__ __launch_bounds__(256) void k_part_copy(const char *__restrict__ text, const unsigned long long *__restrict__ line_off,
                                                   int n_lines, const uint8_t *__restrict__ keep,
                                                   const unsigned long long *__restrict__ kept_off, char *__restrict__ out,
                                                   unsigned long long *__restrict__ kept_bytes) {
    const unsigned long long base = line_off[0], K = kept_off[n_lines];
    if (blockIdx.x == 0 && threadIdx.x == 0 && kept_bytes) *kept_bytes = K;
    const unsigned long long mean = (line_off[n_lines] - base) / (unsigned long long)n_lines;
    int T = 1;
    while (T < 64 && 64ull * (unsigned long long)T < mean) T <<= 1;
    const int lane = (int)(threadIdx.x & 63), per_wave = 64 / T;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (blockDim.x >> 6) * per_wave;
    for (long long i = wave * per_wave + lane / T; i < n_lines; i += stride) {
        const unsigned long long lo = line_off[i], n = line_off[i + 1] - lo, ko = kept_off[i];
        const unsigned long long d = keep[i] ? ko : K + (lo - base) - ko;
        part_copy_line<ALIGNED_LOADS>(text + lo, out + d, n, lane & (T - 1), T);
    }
}


// ---- the multi-way form (hpgv_lines_multisplit_dev, hpgv_text_multisplit; the split tool, hpg-var-vcf split): bucket b's
// lines back to back in line order from bucket_off[b], the buckets in id order; a line whose id is >= n_buckets goes nowhere.
//
//   k_msplit_tile_sums                          : tiles of 64 lines, one wave each.  tile_sum[b][t] = the bytes of bucket b in
//                                                 tile t; in_tile[i] = the bytes of the earlier lines of i's tile in i's bucket
//                                                 (one readlane loop over the 64 lanes, whatever n_buckets is)
//   k_mtile_sums / k_head_bases / k_mtile_offsets : tile_base = exclusive sum of tile_sum in bucket-major order (the same
//                                                 three-launch scan, over n_buckets x n_tiles entries), tile_base[nb nt] = end
//   k_msplit_copy                               : line i to tile_base[b][i / 64] + in_tile[i] by part_copy_line, as k_part_copy
static __global__ __launch_bounds__(256) void k_msplit_tile_sums(const unsigned long long *__restrict__ line_off, const uint8_t *__restrict__ bucket,
                                                                 int n_lines, int n_buckets, int n_tiles,
                                                                 unsigned long long *__restrict__ tile_sum, unsigned long long *__restrict__ in_tile) {
    const int lane = (int)(threadIdx.x & 63);
    const int tile = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (tile >= n_tiles) return;                                    // (a whole wave)
    const long long i = (long long)tile * 64 + lane;
    const unsigned id = i < n_lines ? (unsigned)bucket[i] : 0xFFFFFFFFu;
    const unsigned long long len = id < (unsigned)n_buckets ? line_off[i + 1] - line_off[i] : 0ull;
    unsigned long long off = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;     // s_q: bucket lane + 64 q of this tile
    const unsigned len_lo = (unsigned)len, len_hi = (unsigned)(len >> 32);
    for (int j = 0; j < 64; ++j) {
        const unsigned idj = (unsigned)__builtin_amdgcn_readlane((int)id, j);
        const unsigned long long lj = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)len_lo, j)
                                    | ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)len_hi, j) << 32);
        if (j < lane && idj == id) off += lj;
        const unsigned d = idj - (unsigned)lane;                    // lanes of a dropped id carry 0 bytes
        if (d == 0) s0 += lj; else if (d == 64) s1 += lj; else if (d == 128) s2 += lj; else if (d == 192) s3 += lj;
    }
    if (i < n_lines) in_tile[i] = off;
    const size_t nt = (size_t)n_tiles;
    if (lane < n_buckets) tile_sum[(size_t)lane * nt + tile] = s0;
    if (lane + 64 < n_buckets) tile_sum[(size_t)(lane + 64) * nt + tile] = s1;
    if (lane + 128 < n_buckets) tile_sum[(size_t)(lane + 128) * nt + tile] = s2;
    if (lane + 192 < n_buckets) tile_sum[(size_t)(lane + 192) * nt + tile] = s3;
}

struct TileLen {
    const unsigned long long *__restrict__ tile_sum;
    __device__ __forceinline__ unsigned long long operator()(int i) const { return tile_sum[i]; }
};
static __global__ __launch_bounds__(1024) void k_mtile_sums(const unsigned long long *__restrict__ tile_sum, int n, unsigned long long *__restrict__ block_sum) {
    len_block_sums(TileLen{tile_sum}, n, block_sum);
}
static __global__ __launch_bounds__(1024) void k_mtile_offsets(const unsigned long long *__restrict__ tile_sum, int n,
                                                               const unsigned long long *__restrict__ block_base,
                                                               unsigned long long *__restrict__ tile_base) {
    len_offsets(TileLen{tile_sum}, n, block_base, tile_base);
}

// lanes per line and the grid as k_part_copy; block 0 also writes bucket_off (bucket b starts at its tile 0's base)
static __global__ __launch_bounds__(256) void k_msplit_copy(const char *__restrict__ text, const unsigned long long *__restrict__ line_off,
                                                     int n_lines, const uint8_t *__restrict__ bucket, int n_buckets, int n_tiles,
                                                     const unsigned long long *__restrict__ tile_base,
                                                     const unsigned long long *__restrict__ in_tile, char *__restrict__ out,
                                                     unsigned long long *__restrict__ bucket_off) {
    const size_t nt = (size_t)n_tiles;
    if (blockIdx.x == 0)
        for (int b = (int)threadIdx.x; b <= n_buckets; b += (int)blockDim.x) bucket_off[b] = tile_base[(size_t)b * nt];
    const unsigned long long mean = (line_off[n_lines] - line_off[0]) / (unsigned long long)n_lines;
    int T = 1;
    while (T < 64 && 64ull * (unsigned long long)T < mean) T <<= 1;
    const int lane = (int)(threadIdx.x & 63), per_wave = 64 / T;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long stride = (long long)gridDim.x * (blockDim.x >> 6) * per_wave;
    for (long long i = wave * per_wave + lane / T; i < n_lines; i += stride) {
        const unsigned id = bucket[i];
        if (id >= (unsigned)n_buckets) continue;                   // (the whole team: one line)
        const unsigned long long lo = line_off[i], n = line_off[i + 1] - lo;
        const unsigned long long d = tile_base[(size_t)id * nt + (size_t)(i >> 6)] + in_tile[i];
        part_copy_line<0>(text + lo, out + d, n, lane & (T - 1), T);
    }
}

}  // namespace hpgv
