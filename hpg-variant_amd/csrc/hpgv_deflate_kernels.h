// hpgv_deflate_kernels.h -- BGZF members written on the device (hpgv_bgzf_deflate_dev): the text of every segment cut into
// blocks of at most DFL_BLOCK bytes, each block a complete member (18-byte header, raw DEFLATE, CRC-32, ISIZE), the members
// back to back in segment order.  What the filter and split runners write with HPGV_OUT_BGZF.
//
//   k_dfl_seg_sums / k_head_bases / k_dfl_seg_offsets : seg_blk[s] = exclusive sum of the segments' block counts (the heads'
//                                                 three-launch scan, hpgv_text_kernels.h, over another length)
//   k_bgzf_deflate                              : one wave per block, whole member into the block's worst-case slot
//   k_dfl_member_offsets                        : moff[b] = exclusive sum of the member lengths.  The number of blocks is only
//                                                 known on the device, so one workgroup walks them 1024 at a time
//   k_dfl_copy                                  : slot b to d_out + moff[b] by part_copy_line, as k_part_copy; seg_out_off
//
// The compressor: LZ77 with ONE probe per position and fixed Huffman codes (BTYPE 1).  The wave takes 64 consecutive
// positions at a time.  Every lane hashes the four bytes at its position, reads the last earlier position with that hash
// out of an LDS table (2 048 entries; the lanes of a window then enter their own positions, the highest one winning by
// ds_max), checks the candidate's four bytes and extends the match eight bytes per step out of the cache.  The greedy parse
// of the window is serial and wave-uniform (one readlane per token: a match jumps over the lanes it covers, and the next
// window begins where the last token ends); the tokens' code lengths are prefix-summed across the wave, their bits are
// ORed into 64 words of LDS, and the full words go out in one dword store per window.  A member whose payload would be no
// smaller than its text is written stored (BTYPE 0): never more than 65 311 bytes.  Nothing depends on the order in which
// waves run: the same text gives the same bytes.
// Included by hpgv_deflate_capi.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hpgv_text_kernels.h"
#include "hpgv_partition_kernels.h"
#include "hpgv_crc_kernels.h"

namespace hpgv {

enum { DFL_BLOCK = 65280,                  // text bytes per member (what bgzip writes)
       DFL_SLOT = 66048,                   // scratch per block: 2 unused bytes, the header, then the payload on a dword boundary
       DFL_MEMBER = 2, DFL_PAY = 20,
       DFL_HASH_BITS = 11, DFL_MIN_MATCH = 4, DFL_MAX_MATCH = 258, DFL_MAX_DIST = 32768,
       DFL_OVERHEAD = 18 + 5 + 8 };        // a stored member beyond its text
// a window adds at most 64 x 31 bits to a payload that had at most 8 bits per text byte before it
static_assert(DFL_PAY + DFL_BLOCK + 64 * 31 / 8 + 8 + 8 <= DFL_SLOT, "a slot holds what a block's last window may write");

typedef uint32_t dfl_u32_u __attribute__((aligned(1)));
typedef uint64_t dfl_u64_u __attribute__((aligned(1)));

__host__ __device__ inline size_t dfl_round256(size_t x) { return (x + 255) & ~(size_t)255; }
// scratch: seg_blk[n_segs + 1] and its scan's block sums | moff[nb + 1], mlen[nb] | nb slots (nb = seg_blk[n_segs])
__host__ __device__ inline size_t dfl_head_bytes(int n_segs) {
    return dfl_round256(((size_t)n_segs + 1 + ((size_t)n_segs + 1023) / 1024) * sizeof(unsigned long long));
}
__host__ __device__ inline size_t dfl_meta_bytes(unsigned long long nb) { return dfl_round256((2 * (size_t)nb + 1) * sizeof(unsigned long long)); }
struct DflLayout { unsigned long long nb, *moff, *mlen; uint8_t *slots; };
__device__ __forceinline__ DflLayout dfl_layout(void *scratch, int n_segs) {
    DflLayout L;
    L.nb = ((const unsigned long long *)scratch)[n_segs];
    char *p = (char *)scratch + dfl_head_bytes(n_segs);
    L.moff = (unsigned long long *)p; L.mlen = L.moff + L.nb + 1;
    L.slots = (uint8_t *)(p + dfl_meta_bytes(L.nb));
    return L;
}

struct SegBlocks {
    const unsigned long long *__restrict__ seg_off;
    __device__ __forceinline__ unsigned long long operator()(int s) const { return (seg_off[s + 1] - seg_off[s] + (DFL_BLOCK - 1)) / DFL_BLOCK; }
};
static __global__ __launch_bounds__(1024) void k_dfl_seg_sums(const unsigned long long *__restrict__ seg_off, int n_segs, unsigned long long *__restrict__ block_sum) {
    len_block_sums(SegBlocks{seg_off}, n_segs, block_sum);
}
static __global__ __launch_bounds__(1024) void k_dfl_seg_offsets(const unsigned long long *__restrict__ seg_off, int n_segs,
                                                                 const unsigned long long *__restrict__ block_base, unsigned long long *__restrict__ seg_blk) {
    len_offsets(SegBlocks{seg_off}, n_segs, block_base, seg_blk);
}

__device__ __forceinline__ uint32_t dfl_rev(uint32_t code, int bits) { return __brev(code) >> (32 - bits); }
// the fixed-Huffman bits of one token, least significant bit first out: a literal (len < DFL_MIN_MATCH) or a match
__device__ __forceinline__ void dfl_token(uint32_t lit, uint32_t len, uint32_t dist, uint32_t *code, uint32_t *bits) {
    if (len < (uint32_t)DFL_MIN_MATCH) {
        if (lit < 144u) { *code = dfl_rev(0x30u + lit, 8); *bits = 8; }
        else { *code = dfl_rev(0x190u + lit - 144u, 9); *bits = 9; }
        return;
    }
    const uint32_t l = len - 3;
    uint32_t sym, xb = 0, xv = 0;
    if (len == (uint32_t)DFL_MAX_MATCH) sym = 285;
    else if (l < 8u) sym = 257 + l;
    else { xb = (31u - (uint32_t)__clz((int)l)) - 2u; sym = 261 + 4 * xb + ((l >> xb) & 3u); xv = l & ((1u << xb) - 1u); }
    uint32_t c, n;
    if (sym < 280u) { c = dfl_rev(sym - 256u, 7); n = 7; } else { c = dfl_rev(0xC0u + sym - 280u, 8); n = 8; }
    c |= xv << n; n += xb;
    const uint32_t d = dist - 1;
    uint32_t dc = d, dxb = 0, dxv = 0;
    if (d >= 4u) { const uint32_t k = 31u - (uint32_t)__clz((int)d); dxb = k - 1; dc = 2 * k + ((d >> dxb) & 1u); dxv = d & ((1u << dxb) - 1u); }
    c |= dfl_rev(dc, 5) << n; n += 5;
    c |= dxv << n; n += dxb;
    *code = c; *bits = n;                                           // at most 8 + 5 + 5 + 13 = 31
}

// one block: the n bytes at p (1 .. DFL_BLOCK) as a member from slot + DFL_MEMBER on; returns the member's length.  One wave
// (a workgroup of its own: the barriers below order its LDS traffic), s_hash[1 << DFL_HASH_BITS], s_bits[64].
__device__ __forceinline__ uint32_t dfl_one_block(const uint8_t *__restrict__ p, const uint32_t n, uint8_t *__restrict__ slot,
                                                  const uint32_t *s_tab, uint32_t *s_hash, uint32_t *s_bits) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t crc = crc_wave(s_tab, p, n);
    for (uint32_t i = lane; i < (1u << DFL_HASH_BITS); i += 64) s_hash[i] = 0;      // position + 1 (0: none yet)
    s_bits[lane] = lane == 0 ? 3u : 0u;                             // BFINAL 1, BTYPE 01
    __syncthreads();
    uint32_t *pay = (uint32_t *)(slot + DFL_PAY);
    uint32_t nbits = 3, outw = 0, pos = 0;                          // bits waiting in s_bits (< 32 between windows), words stored, next position
    bool stored = false;
    while (pos < n) {
        const uint32_t q = pos + lane;
        const bool can = q + 4 <= n;                                // four bytes to hash inside the block
        uint32_t w4 = 0, h = 0, len = 0, dist = 0;
        if (can) { w4 = *(const dfl_u32_u *)(p + q); h = (w4 * 2654435761u) >> (32 - DFL_HASH_BITS); }
        else if (q < n) w4 = p[q];
        const uint32_t seen = can ? s_hash[h] : 0u;
        __syncthreads();                                            // every lane has read the table before the window is entered
        if (can) atomicMax(&s_hash[h], q + 1);
        if (seen) {
            const uint32_t c = seen - 1;                            // c < pos: entered by an earlier window
            if (q - c <= (uint32_t)DFL_MAX_DIST && *(const dfl_u32_u *)(p + c) == w4) {
                const uint32_t maxl = n - q < (uint32_t)DFL_MAX_MATCH ? n - q : (uint32_t)DFL_MAX_MATCH;
                uint32_t l = 4;
                bool open = true;
                while (open && l + 8 <= maxl) {                     // (q + l + 8 <= n: no load leaves the block)
                    const uint64_t x = *(const dfl_u64_u *)(p + q + l) ^ *(const dfl_u64_u *)(p + c + l);
                    if (x) { l += (uint32_t)__builtin_ctzll(x) >> 3; open = false; } else l += 8;
                }
                while (open && l < maxl && p[q + l] == p[c + l]) ++l;
                len = l; dist = q - c;
            }
        }
        // the greedy parse: lane 0 starts a token, and so does the lane behind every token's last byte
        const uint32_t span = len >= (uint32_t)DFL_MIN_MATCH ? len : 1u;
        const uint32_t wlen = n - pos < 64u ? n - pos : 64u;
        uint64_t starts = 0;
        uint32_t c = 0;
        while (c < wlen) { starts |= 1ull << c; c += (uint32_t)__builtin_amdgcn_readlane((int)span, (int)c); }
        uint32_t code = 0, tb = 0;
        if ((starts >> lane) & 1ull) dfl_token(w4 & 0xFFu, len, dist, &code, &tb);
        uint32_t inc = tb;
        for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off); if (lane >= (uint32_t)off) inc += o; }
        const uint32_t total = nbits + (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        if (tb) {
            const uint32_t at = nbits + inc - tb;
            const uint64_t v = (uint64_t)code << (at & 31u);
            atomicOr(&s_bits[at >> 5], (uint32_t)v);
            if (v >> 32) atomicOr(&s_bits[(at >> 5) + 1], (uint32_t)(v >> 32));
        }
        __syncthreads();
        const uint32_t nfull = total >> 5;                          // at most (31 + 64 x 31) / 32 = 62
        if (lane < nfull) pay[outw + lane] = s_bits[lane];
        const uint32_t rest = s_bits[nfull];
        __syncthreads();
        s_bits[lane] = lane == 0 ? rest : 0u;
        __syncthreads();
        outw += nfull; nbits = total & 31u; pos += c;
        if ((uint64_t)outw * 32 + nbits > 8ull * n) { stored = true; break; }       // already no smaller than the text
    }
    uint32_t P = 0;                                                 // payload bytes
    if (!stored) {
        const uint32_t t = nbits + 7;                               // the end-of-block code: seven zero bits
        P = outw * 4 + ((t + 7) >> 3);
        if (P >= n) stored = true;
        else if (lane < ((t + 31) >> 5)) pay[outw + lane] = s_bits[lane];
    }
    __syncthreads();
    if (stored) {
        uint8_t *o = slot + DFL_PAY;
        if (lane == 0) { o[0] = 1; o[1] = (uint8_t)n; o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~n; o[4] = (uint8_t)(~n >> 8); }
        part_copy_line<0>((const char *)p, (char *)o + 5, n, (int)lane, 64);
        P = n + 5;
    }
    const uint32_t bsize = P + 25;                                  // member length - 1
    if (lane < 18) {
        const uint32_t hdr = lane == 0 ? 0x1Fu : lane == 1 ? 0x8Bu : lane == 2 ? 8u : lane == 3 ? 4u : lane == 9 ? 0xFFu : lane == 10 ? 6u
                           : lane == 12 ? 0x42u : lane == 13 ? 0x43u : lane == 14 ? 2u : lane == 16 ? bsize & 0xFFu : lane == 17 ? bsize >> 8 : 0u;
        slot[DFL_MEMBER + lane] = (uint8_t)hdr;
    }
    if (lane < 8) slot[DFL_PAY + P + lane] = (uint8_t)((lane < 4 ? crc : n) >> (8 * (lane & 3)));      // behind the payload's last word
    return bsize + 1;
}

// a grid of single waves striding over the blocks (their number is on the device): block b is bytes [k DFL_BLOCK, ...) of its
// segment, the segment found by bisection of seg_blk
static __global__ __launch_bounds__(64) void k_bgzf_deflate(const uint8_t *__restrict__ text, const unsigned long long *__restrict__ seg_off,
                                                            int n_segs, void *scratch, const uint32_t *__restrict__ tab) {
    __shared__ uint32_t s_tab[CRC_TAB_WORDS];
    __shared__ uint32_t s_hash[1 << DFL_HASH_BITS];
    __shared__ uint32_t s_bits[64];
    const DflLayout L = dfl_layout(scratch, n_segs);
    if ((unsigned long long)blockIdx.x >= L.nb) return;
    for (int i = threadIdx.x; i < CRC_TAB_WORDS; i += 64) s_tab[i] = tab[i];
    __syncthreads();
    const unsigned long long *seg_blk = (const unsigned long long *)scratch;
    for (unsigned long long b = blockIdx.x; b < L.nb; b += gridDim.x) {
        int lo = 0, hi = n_segs;                                    // the last s with seg_blk[s] <= b (seg_blk[n_segs] = nb > b)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg_blk[mid] <= b) lo = mid; else hi = mid; }
        const unsigned long long from = seg_off[lo] + (b - seg_blk[lo]) * DFL_BLOCK, left = seg_off[lo + 1] - from;
        const uint32_t n = left < (unsigned long long)DFL_BLOCK ? (uint32_t)left : (uint32_t)DFL_BLOCK;
        const uint32_t m = dfl_one_block(text + from, n, L.slots + (size_t)b * DFL_SLOT, s_tab, s_hash, s_bits);
        if (threadIdx.x == 0) L.mlen[b] = m;
        __syncthreads();
    }
}

static __global__ __launch_bounds__(1024) void k_dfl_member_offsets(void *scratch, int n_segs) {
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned long long carry;
    const DflLayout L = dfl_layout(scratch, n_segs);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (unsigned long long b0 = 0; b0 < L.nb; b0 += 1024) {        // exclusive, 1024 members per turn
        const unsigned long long b = b0 + threadIdx.x;
        const unsigned long long v = b < L.nb ? L.mlen[b] : 0ull;
        const unsigned long long inc = head_block_scan(v, s_w);
        const unsigned long long base = carry;
        if (b < L.nb) L.moff[b] = base + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = base + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) L.moff[L.nb] = carry;
}

// whole waves striding over the members, a wave per member; block 0 also writes seg_out_off (segment s starts at its first
// block's member)
static __global__ __launch_bounds__(256) void k_dfl_copy(void *scratch, int n_segs, uint8_t *__restrict__ out, unsigned long long *__restrict__ seg_out_off) {
    const DflLayout L = dfl_layout(scratch, n_segs);
    const unsigned long long *seg_blk = (const unsigned long long *)scratch;
    if (blockIdx.x == 0)
        for (int s = (int)threadIdx.x; s <= n_segs; s += (int)blockDim.x) seg_out_off[s] = L.moff[seg_blk[s]];
    const int lane = (int)(threadIdx.x & 63);
    const unsigned long long wave = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned long long stride = (unsigned long long)gridDim.x * (blockDim.x >> 6);
    for (unsigned long long b = wave; b < L.nb; b += stride)
        part_copy_line<0>((const char *)L.slots + (size_t)b * DFL_SLOT + DFL_MEMBER, (char *)out + L.moff[b], L.mlen[b], lane, 64);
}

}  // namespace hpgv
