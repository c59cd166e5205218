// hpgv_inherit_kernels.h -- the inheritance scan behind the --inh-dom / --inh-rec record filters
// (shared_options.c:42-56; the filter bodies live in hpg-libs, these definitions are this project's: include/hpgv.h).
//
// Input: rows of HPGV_LAYOUT_ASSOC ([affected | pad16 | unaffected | pad .. pitch), pad bytes 0xFF).  The scan has the
// shape of the other count scans (hpgv_kernels.h): one row per wavefront, 16 B per lane per load, SWAR on the nibbles,
// DPP + readlane wave reduction, one 32-byte store per row.  No LDS, no MFMA.
//
// A call is COUNTED when neither allele nibble is 0xF (0xFF and half-missing bytes are not).  Per 4 bytes, with bit 3 of
// every byte as the flag:
//   counted = nib_not_f(w) & (nib_not_f(w) >> 4)
//   non-ref = counted & (nib_nonzero(w) | nib_nonzero(w) >> 4)      byte != 0x00
//   both    = counted & nib_nonzero(w) & (nib_nonzero(w) >> 4)      both alleles non-reference
// Per variant, 8 x int32:
//   {affected counted, affected non-ref, affected both, unaffected counted, unaffected 0/0, unaffected both, 0, 0}
// with unaffected 0/0 = unaffected counted - unaffected non-ref.  Multi-allelic codes count by the same rules.
//
// Per-lane partial sums of the two classes share one register (affected in bits 0..15, unaffected in bits 16..31) and
// are unpacked before the wave reduction.  A lane sees at most pitch / 16 / 64 + 1 chunks of a row, 16 calls each, and
// the cohort's pitch is capped (pitch_supported: pitch / 16 / 64 <= 2030), so a half holds at most 32 496: no overflow,
// whatever the class sizes (a class of 65 536 samples or more gives a lane about 1 100).
#pragma once
#include "hpgv_kernels.h"

namespace hpgv {

template <bool NT, int U>
__global__ __launch_bounds__(256) void k_inherit_scan(const uint8_t *__restrict__ gt, size_t pitch, int n_variants,
                                                      int chunksA, int chunks, int4 *__restrict__ counts, int vpw) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long v0 = wave * vpw;
    const long v_end = v0 + vpw < n_variants ? v0 + vpw : n_variants;
    for (long v = v0; v < v_end; ++v) {                                 // wave-uniform
        const uint8_t *row = gt + (size_t)v * pitch;
        uint32_t pc = 0, pn = 0, pb = 0;                                // counted, non-ref, both: affected | unaffected << 16
        for (int base = 0; base < chunks; base += 64 * U) {
            uint4 q[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = base + u * 64 + lane;
                q[u] = make_uint4(~0u, ~0u, ~0u, ~0u);                  // past the row: all missing, counts nothing
                if (c < chunks) q[u] = load16o<NT>(row, (uint32_t)c * 16u);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = base + u * 64 + lane;
                const uint32_t sh = (c < chunksA) ? 0u : 16u;
                const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                uint32_t nc = 0, nn = 0, nb = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t f = nib_not_f(w[k]), z = nib_nonzero(w[k]);
                    const uint32_t cnt = f & (f >> 4) & 0x08080808u;
                    nc += __builtin_popcount(cnt);
                    nn += __builtin_popcount((z | (z >> 4)) & cnt);
                    nb += __builtin_popcount(z & (z >> 4) & cnt);
                }
                pc += nc << sh;
                pn += nn << sh;
                pb += nb << sh;
            }
        }
        const int cA = wave_sum((int)(pc & 0xFFFFu)), cU = wave_sum((int)(pc >> 16));
        const int nA = wave_sum((int)(pn & 0xFFFFu)), nU = wave_sum((int)(pn >> 16));
        const int bA = wave_sum((int)(pb & 0xFFFFu)), bU = wave_sum((int)(pb >> 16));
        // lanes 0 and 1 store the two halves of the row's 32 bytes: one store instruction
        if (lane < 2) counts[2 * v + lane] = lane == 0 ? make_int4(cA, nA, bA, cU) : make_int4(cU - nU, bU, 0, 0);
    }
}

// the verdict of --inh-dom / --inh-rec from the counts (a negative threshold: that filter off):
//   dominant followers  = c1 + c4,  recessive followers = c2 + (c3 - c5),  fraction = followers / (c0 + c3) in double;
//   kept when every active fraction >= its threshold; a record with no counted call fails
static __global__ __launch_bounds__(256) void k_inherit_filter(const int4 *__restrict__ in8, int n, double min_dom,
                                                               double min_rec, uint8_t *__restrict__ keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 lo = in8[2 * i], hi = in8[2 * i + 1];
    const int c0 = lo.x, c1 = lo.y, c2 = lo.z, c3 = lo.w, c4 = hi.x, c5 = hi.y;
    const int den = c0 + c3;
    bool ok = den > 0;
    if (ok && min_dom >= 0.0) ok = (double)(c1 + c4) / (double)den >= min_dom;
    if (ok && min_rec >= 0.0) ok = (double)(c2 + (c3 - c5)) / (double)den >= min_rec;
    keep[i] = ok ? 1 : 0;
}

}  // namespace hpgv
