// hpgv_tdt_perm_kernels.h -- max(T) permutation of the TDT by family flips on the matrix cores (gfx950).
//
// Family f contributes (t1_f, t2_f) to a variant's {t1, t2}.  A permutation flips "transmitted" and "untransmitted" for all
// children of a family at once: under a sign vector s_p in {+1, -1}^families a flipped family contributes (t2_f, t1_f).  So
//     t1_p + t2_p = t1 + t2 = n                     is invariant, and
//     t1_p - t2_p = D_p = sum_f s_p(f) d_f          with d_f = t1_f - t2_f
// is a [variants x families] x [families x permutations] i8 product with exact i32 sums, v_mfma_i32_16x16x64_i8; the permuted
// counts are {(n + D_p) / 2, (n - D_p) / 2}, integral because t1_f + t2_f and t1_f - t2_f have the same parity.
//
// One signed plane.  d is carried as ONE i8 plane (tdt4_diff: per-byte popcounts of the two masked pair words and a borrow-safe
// SWAR subtraction), not as two unsigned planes pc(w1), pc(w2) with an accumulator each as k_assoc_perm carries c1 / c2: the
// statistic needs only the difference (the sum is the observed one), the operand is signed i8 anyway, and one plane is half
// the MFMAs and half the accumulator registers for three more vector operations per dword.
//
// K positions.  0 .. P16 - 1: the fast trios in plane order -- trio t is byte t of the father, mother and child planes
// (TdtPlan::build), so the 16 bytes a lane loads from each plane are 16 consecutive k values of one variant, and a lane turns
// them into one A fragment in registers.  P16 .. P16 + n_slow - 1: the families with several counted children, padded to a
// multiple of 16.  Their d_f = t1_f - t2_f of tdt_family_slow (|d_f| <= 2 x children: at most 63 children fit i8) is written
// by a pre-pass, k_tdt_perm_slow, one lane per (variant, slow family), as an i8 tail [variants x round16(n_slow)]; the product
// kernel reads that tail as ordinary A fragments after the planes, which keeps a scalar loop over 16 families per lane out of
// it.  A pad trio inside the planes decodes to d = 0 as it does to {0, 0} in k_tdt_scan, chunks past the tail are zeros, and
// the sign matrix [round16(n_perms) x K pitch] holds +1 / -1 under a family and 0 under every pad and in the rows past
// n_perms, in the same K order: the 16 bytes a lane takes of it are the B fragment over the SAME 16 k values.
//
// Lane maps, tile and staging are k_assoc_perm's (hpgv_assoc_perm_kernels.h): A and B, lane l holds row / column l & 15 and
// the 16 k values of lane group l >> 4; C/D, col = l & 15 (permutation), row = (l >> 4) * 4 + reg (variant).  A workgroup of
// four waves owns PERM_VT = 64 variants x PERM_PT = 128 permutations; per k-step of 64 positions a wave loads its genotype
// bytes once and runs PERM_PT / 16 MFMAs against the k-step's sign tile, staged in LDS in two buffers (one barrier per k-step).
//
// Grid.  A launch reads the rows of a variant tile once per pass (ceil(n_perms / 128) passes), three planes each: three times
// the label kernel's bytes per k.  The grid is therefore one-dimensional with the passes of a tile 8 workgroups apart
// (workgroup b: tile = (b / 8 / passes) * 8 + b % 8, pass = (b / 8) % passes): workgroups are dealt to the 8 XCDs in turn, so
// the passes of a tile start together and share one L2 instead of each fetching the tile's rows from memory (3.82 -> 2.32 ms
// on the shape of profiles/tdt_perm.json).  This is a matter of speed alone: any placement gives the same sums.  The grid is
// rounded up to 8 tiles; workgroups past the last tile leave at once.
//
// Epilogue.  Per (variant, permutation) the chi-square of {(n + D_p) / 2, (n - D_p) / 2} by tdt_chisq_value, the device function
// of k_tdt_stats, compared with the observed one.  A variant with n = 0 (chi-square -1) or one flagged in `skip` takes no part:
// n_ge stays 0 and nothing enters the maxima.  Row sums and the merge of the maxima as in k_assoc_perm: the values are >= +0
// there, so the order of the f64 bit patterns read as unsigned integers is the numeric one.
#pragma once
#include "hpgv_assoc_perm_kernels.h"
#include "hpgv_tdt_stats_kernels.h"

namespace hpgv {

// d_f of the slow families of every variant: tail[v * tail_pitch + k], k < tail_pitch = round16(n_slow); 0 for k >= n_slow
static __global__ __launch_bounds__(256) void k_tdt_perm_slow(const uint8_t *__restrict__ gt, size_t pitch, int n_variants, int n_slow,
                                                              int tail_pitch, const int32_t *__restrict__ slow_off,
                                                              const uint8_t *__restrict__ slow_male, int slow_base,
                                                              const uint8_t *__restrict__ is_x, int8_t *__restrict__ tail) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t v = i / (size_t)tail_pitch;
    const int k = (int)(i - v * (size_t)tail_pitch);
    if (v >= (size_t)n_variants) return;
    int d = 0;
    if (k < n_slow) {
        const int off = slow_off[k], n_children = slow_off[k + 1] - off - 2;
        const bool x_row = is_x != nullptr && is_x[v] != 0;
        const int2 t = tdt_family_slow(gt + v * pitch + slow_base + off, n_children, slow_male + off, x_row);
        d = t.x - t.y;
    }
    tail[i] = (int8_t)d;
}

struct TdtPermArgs {
    const uint8_t *gt;               // tdt layout, rows `pitch` bytes apart
    size_t pitch;
    int pchunks;                     // P16 / 16: chunks of the three planes
    int kchunks;                     // K pitch / 16 = pchunks + tail_pitch / 16
    int n_variants;
    const uint8_t *is_x;             // per variant, may be null
    TdtLuts luts;
    const uint8_t *male_plane;       // 0xFF per male child of the fast trios
    const int8_t *tail;              // k_tdt_perm_slow's output; null without slow families
    int tail_pitch;
    const int2 *tu;                  // observed {t1, t2} of hpgv_tdt_scan_dev
    const uint8_t *signs;            // [sign_rows x kchunks * 16] i8 +1 / -1, 0 under the pads
    int n_perms, sign_rows;
    int passes;                      // ceil(n_perms / PERM_PT)
    const uint8_t *skip;             // per variant, may be null: != 0 = the row takes no part (n_ge stays 0)
    int *n_ge;                       // [n_variants], zeroed before the launch
    unsigned long long *batch_max;   // [n_perms] f64 bit patterns, zeroed before the launch
    int *perm_tu;                    // [(v * n_perms + p) * 2 + k] or null
};

// the bytes a lane needs for its chunk of a k-step: the three planes' (and, on a chr X row, the male plane's), or the tail's in f
struct TdtPermRaw { uint4 f, m, c, ml; };

__global__ __launch_bounds__(256) void k_tdt_perm(const TdtPermArgs A) {
    __shared__ uint4 sgn[2][PERM_PT * PERM_LDS_ROW];
    __shared__ unsigned long long wg_max[PERM_PT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    // workgroup -> (variant tile, pass), see "Grid" above: the passes of a tile are the workgroups 8 apart
    const unsigned seq = blockIdx.x >> 3;
    const int tile = (int)(seq / (unsigned)A.passes) * 8 + (int)(blockIdx.x & 7u);
    if ((long)tile * PERM_VT >= A.n_variants) return;                           // (the whole workgroup: the grid is rounded up to 8 tiles)
    const int p0 = (int)(seq % (unsigned)A.passes) * PERM_PT;
    const int v_lane = tile * PERM_VT + wave * 16 + col;                   // the variant whose bytes this lane loads
    const bool v_ok = v_lane < A.n_variants;
    const bool x = v_ok && A.is_x != nullptr && A.is_x[v_lane] != 0;
    const uint8_t *row = A.gt + (size_t)(v_ok ? v_lane : 0) * A.pitch;
    const uint8_t *trow = reinterpret_cast<const uint8_t *>(A.tail) + (size_t)(v_ok ? v_lane : 0) * (size_t)A.tail_pitch;
    const uint32_t plane = (uint32_t)A.pchunks * 16u;
    const size_t kpitch = (size_t)A.kchunks * 16;
    const int steps = (A.kchunks + 3) / 4;

    // the sign tile of k-step s: PERM_PT rows x 4 chunks of 16 bytes, two per thread; rows past the matrix and chunks past the
    // K pitch are zeros
    auto sign_chunk = [&](int s, int i) -> uint4 {
        const int r = i >> 2, c = s * 4 + (i & 3);
        if (p0 + r < A.sign_rows && c < A.kchunks)
            return *reinterpret_cast<const uint4 *>(A.signs + (size_t)(p0 + r) * kpitch + (size_t)c * 16);
        return make_uint4(0u, 0u, 0u, 0u);
    };
    auto gt_load = [&](int s) -> TdtPermRaw {
        const int c = s * 4 + kq;
        TdtPermRaw q;
        // the virtual trio of k_tdt_scan: unusable parents, missing child
        q.f = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        q.m = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
        q.c = make_uint4(0x04040404u, 0x04040404u, 0x04040404u, 0x04040404u);
        q.ml = make_uint4(0u, 0u, 0u, 0u);
        if (v_ok && c < A.pchunks) {
            q.f = load16o<false>(row, (uint32_t)c * 16u);
            q.m = load16o<false>(row, (uint32_t)c * 16u + plane);
            q.c = load16o<false>(row, (uint32_t)c * 16u + 2u * plane);
            if (x) q.ml = reinterpret_cast<const uint4 *>(A.male_plane)[c];
        } else if (v_ok && c < A.kchunks) {
            q.f = load16o<false>(trow, (uint32_t)(c - A.pchunks) * 16u);
        }
        return q;
    };
    // the A fragment of the lane's chunk: 16 i8 differences
    auto gt_diff = [&](int s, const TdtPermRaw &q) -> perm_i32x4 {
        const int c = s * 4 + kq;
        perm_i32x4 a = {0, 0, 0, 0};
        if (c < A.pchunks) {
            if (x) {
                a[0] = (int)tdt4_diff<true>(A.luts, q.f.x, q.m.x, q.c.x, q.ml.x); a[1] = (int)tdt4_diff<true>(A.luts, q.f.y, q.m.y, q.c.y, q.ml.y);
                a[2] = (int)tdt4_diff<true>(A.luts, q.f.z, q.m.z, q.c.z, q.ml.z); a[3] = (int)tdt4_diff<true>(A.luts, q.f.w, q.m.w, q.c.w, q.ml.w);
            } else {
                a[0] = (int)tdt4_diff<false>(A.luts, q.f.x, q.m.x, q.c.x, 0); a[1] = (int)tdt4_diff<false>(A.luts, q.f.y, q.m.y, q.c.y, 0);
                a[2] = (int)tdt4_diff<false>(A.luts, q.f.z, q.m.z, q.c.z, 0); a[3] = (int)tdt4_diff<false>(A.luts, q.f.w, q.m.w, q.c.w, 0);
            }
        } else if (v_ok && c < A.kchunks) {
            a[0] = (int)q.f.x; a[1] = (int)q.f.y; a[2] = (int)q.f.z; a[3] = (int)q.f.w;
        }
        return a;
    };
    constexpr int LPT = PERM_PT * 4 / 256;                                 // sign chunks per thread and k-step
    static_assert(PERM_PT * 4 % 256 == 0, "the sign tile is staged by 256 threads");

    perm_i32x4 acc[PERM_NT];
#pragma unroll
    for (int n = 0; n < PERM_NT; ++n) acc[n] = perm_i32x4{0, 0, 0, 0};
    if (tid < PERM_PT) wg_max[tid] = 0ull;
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
        const int i = tid + k * 256;
        sgn[0][(i >> 2) * PERM_LDS_ROW + (i & 3)] = sign_chunk(0, i);
    }
    TdtPermRaw g = gt_load(0);
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        TdtPermRaw gn = g;
        uint4 ln[LPT];
        if (more) {
            gn = gt_load(s + 1);
#pragma unroll
            for (int k = 0; k < LPT; ++k) ln[k] = sign_chunk(s + 1, tid + k * 256);
        }
        const perm_i32x4 a = gt_diff(s, g);
        const uint4 *buf = sgn[s & 1];
#pragma unroll
        for (int n = 0; n < PERM_NT; ++n) {
            const uint4 q = buf[(n * 16 + col) * PERM_LDS_ROW + kq];
            const perm_i32x4 b = {(int)q.x, (int)q.y, (int)q.z, (int)q.w};
            acc[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[n], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < LPT; ++k) {
                const int i = tid + k * 256;
                sgn[(s + 1) & 1][(i >> 2) * PERM_LDS_ROW + (i & 3)] = ln[k];
            }
        }
        __syncthreads();
        g = gn;
    }

    // ---- epilogue: acc[n][r] is D_p of variant vr0 + r and permutation p0 + 16 n + col
    const int vr0 = tile * PERM_VT + wave * 16 + kq * 4;
    double pmax[PERM_NT];
#pragma unroll
    for (int n = 0; n < PERM_NT; ++n) pmax[n] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int v = vr0 + r;
        const bool live = v < A.n_variants && !(A.skip != nullptr && A.skip[v] != 0);
        int2 o = make_int2(0, 0);
        if (live) o = A.tu[v];
        const int tot = o.x + o.y;
        const bool ok = live && tot > 0;                                   // nothing transmitted: no statistic, no part
        const double t_obs = tdt_chisq_value(o.x, o.y);
        int cnt = 0;
#pragma unroll
        for (int n = 0; n < PERM_NT; ++n) {
            const int p = p0 + n * 16 + col;
            if (live && p < A.n_perms) {
                const int d = acc[n][r];
                const int t1 = (tot + d) >> 1, t2 = (tot - d) >> 1;       // tot and d have the same parity, |d| <= tot
                if (A.perm_tu != nullptr)
                    *reinterpret_cast<int2 *>(A.perm_tu + ((size_t)v * (size_t)A.n_perms + (size_t)p) * 2) = make_int2(t1, t2);
                if (ok) {
                    const double t = tdt_chisq_value(t1, t2);
                    if (t >= t_obs) ++cnt;
                    if (t > pmax[n]) pmax[n] = t;
                }
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
