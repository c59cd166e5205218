// hpgv_ld_kernels.h -- windowed pairwise r^2 between the rows of one genotype matrix on the matrix cores (gfx950).
//
// For rows a < b with the planes v = valid (0 / 1), g = dosage (0 when missing) and q = g^2 (0, 1 or 4) of their HPGV8 bytes
// (include/hpgv.h "LD") the six moments over the samples called in both rows
//     n = sum v_a v_b    sa = sum g_a v_b    sb = sum v_a g_b    saa = sum q_a v_b    sbb = sum v_a q_b    sab = sum g_a g_b
// are six [variants x samples] x [samples x variants] i8 products with exact i32 sums, v_mfma_i32_16x16x64_i8, restricted to
// the band 1 <= b - a <= window.  This is k_assoc_perm's product (hpgv_assoc_perm_kernels.h) with the label rows replaced by
// other rows of the same matrix.
//
// Lane maps.  A and B: lane l holds row / column l & 15 and the 16 k values of lane group l >> 4; both operands are the bytes
// of the same sample offset k0 + 16 (l >> 4) of their rows, byte for byte, so the sums do not depend on how the hardware
// numbers the k values inside a lane group.  C/D: col = l & 15 (later variant b), row = (l >> 4) * 4 + reg (earlier variant a).
//
// Tile.  A workgroup of four waves owns LD_VT = 64 earlier variants a0 .. a0 + 63 (16 per wave) and one group of LD_BT = 64
// later variants a0 + 64 pass .. a0 + 64 pass + 63; the band of a tile reaches a0 + 63 + window, so a tile takes
// (63 + window) / 64 + 1 passes (pass 0 holds the tile's own triangle).  Per k-step of 64 samples a wave loads its 16 x 64
// genotype bytes from memory once and forms the three A planes in registers; the 64 later rows are staged in LDS AS PLANES: each
// of the 256 threads loads one 16-byte chunk of one later row, forms its three planes once and stores them (3 planes x 64 rows
// x 64 bytes, rows 80 bytes apart, two buffers: one barrier per k-step).  Staging raw bytes instead would make each of the four
// waves form the planes of all 64 rows again after its LDS reads: 16 times the vector work per k-step for a third of the LDS.
// A 16 x 16 block takes six MFMAs per k-step; with 64 later variants a wave holds 4 x 6 accumulators of four registers.  A
// block that lies wholly outside the band (or wholly below b_begin, or past the last row) is skipped for the whole k loop: the
// test is the same for every lane of a wave, so the branch is a scalar one and such a block issues no MFMA.
//
// Grid.  One-dimensional, workgroup w -> (tile, pass).  Workgroups are dealt to the 8 XCDs in turn (w % 8), and an XCD's L2 is
// not shared with the others.  Tile t reads the rows of tiles t .. t + passes - 1, so the tiles are cut into 8 contiguous
// ranges, one per value of w % 8, and within a range the workgroups run tile by tile with a tile's passes next to each other:
// the workgroups in flight on one XCD read one contiguous stretch of rows, and a row is fetched into that L2 once, not once
// per tile that reaches it.  This is a matter of speed alone: any placement gives the same sums.
//
// Epilogue.  Per pair inside the band the six sums, then r^2 by ld_r2_value.  A pair whose rows are skipped, lie on different
// chromosomes or further apart than max_bp gets the quiet NaN and zero counts.  The pairs (b - d, b) with b - d < 0 belong to no
// tile: k_ld_head writes them.
//
// Edge form.  k_ld_edges is the same tile with an epilogue that appends the pairs with r2 >= a threshold to a list and writes no
// band (at the end of this file).
#pragma once
#include "hpgv_assoc_perm_kernels.h"

namespace hpgv {

constexpr int LD_VT = 64;            // earlier variants per workgroup: 16 per wave
constexpr int LD_BT = 64;            // later variants per workgroup and pass
constexpr int LD_NT = LD_BT / 16;
constexpr int LD_LDS_ROW = 5;        // uint4 per staged plane row: 64 bytes + 16 of padding (bank spread of the b128 reads)
constexpr int LD_MAX_WINDOW = 1024;

// r^2 of include/hpgv.h "LD": the three differences exact in int64, the rest f64 in this order (the unit is built with
// -ffp-contract=off).  va == 0 or vb == 0 gives 0 / 0 = NaN
__host__ __device__ inline double ld_r2_value(int n, int sa, int sb, int saa, int sbb, int sab) {
    const long long cov = (long long)n * sab - (long long)sa * sb;
    const long long va = (long long)n * saa - (long long)sa * sa;
    const long long vb = (long long)n * sbb - (long long)sb * sb;
    return ((double)cov * (double)cov) / ((double)va * (double)vb);
}

// what a pair outside the band gets
__device__ __forceinline__ double ld_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// the three planes of 4 packed HPGV8 bytes, one i8 per byte: valid and dosage of perm_planes_trend, q = dosage^2
__device__ __forceinline__ void ld_planes(uint32_t w, uint32_t &v, uint32_t &g, uint32_t &q) {
    perm_planes_trend(w, v, g);
    q = g + (g & 0x02020202u);                          // 0, 1, 2 -> 0, 1, 4
}

struct LdArgs {
    const uint8_t *gt;               // rows of HPGV8 bytes `pitch` apart, pads 0xFF
    size_t pitch;
    int chunks;                      // pitch / 16
    int n_variants;
    int b_begin;                     // later variants below it are not written
    int window;
    int passes;                      // (63 + window) / 64 + 1
    int tiles, tiles_per_range;      // ceil(n_variants / LD_VT); ceil(tiles / 8)
    const int32_t *chrom;            // per row, with pos or null
    const uint32_t *pos;
    long long max_bp;                // < 0: no distance limit
    const uint8_t *skip;             // per row, may be null
    double *r2;                      // [(b - b_begin) * window + (b - a - 1)]
    int32_t *counts6;                // the same index x 6, may be null
};

// the pairs (b - d, b) with d > b: b = b_begin .. min(n_variants, window) - 1; one lane per (b, d)
static __global__ __launch_bounds__(256) void k_ld_head(int b_begin, int b_end, int window, double *__restrict__ r2, int32_t *__restrict__ counts6) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = i / (size_t)window;
    const int d = (int)(i - row * (size_t)window) + 1;
    const int b = b_begin + (int)row;
    if (b >= b_end || d <= b) return;
    r2[i] = ld_nan();
    if (counts6 != nullptr) {
#pragma unroll
        for (int k = 0; k < 6; ++k) counts6[i * 6 + k] = 0;
    }
}

__global__ __launch_bounds__(256) void k_ld_window(const LdArgs A) {
    __shared__ uint4 bt[2][3][LD_BT * LD_LDS_ROW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    // workgroup -> (tile, pass), see "Grid" above
    const int range = (int)(blockIdx.x & 7u);
    const unsigned seq = blockIdx.x >> 3;
    const int in_range = (int)(seq / (unsigned)A.passes), pass = (int)(seq % (unsigned)A.passes);
    const int tile = range * A.tiles_per_range + in_range;
    if (in_range >= A.tiles_per_range || tile >= A.tiles) return;          // (the whole workgroup)
    const int a0 = tile * LD_VT, b0 = a0 + pass * LD_BT;
    // nothing to write: the group lies past the last row or wholly below b_begin
    if (b0 >= A.n_variants || b0 + LD_BT <= A.b_begin) return;

    const int aw = a0 + wave * 16;                                         // the wave's 16 earlier variants
    const int a_lane = aw + col;
    const bool a_ok = a_lane < A.n_variants;
    const uint8_t *arow = A.gt + (size_t)(a_ok ? a_lane : 0) * A.pitch;
    const int steps = (A.chunks + 3) / 4;
    // the chunk of the later rows this thread stages: row tid >> 2 of the group, chunk tid & 3 of the k-step
    const int sr = tid >> 2, sc = tid & 3;
    const bool b_ok = b0 + sr < A.n_variants;
    const uint8_t *brow = A.gt + (size_t)(b_ok ? b0 + sr : 0) * A.pitch;

    // block n of the wave holds the pairs (aw .. aw + 15) x (b0 + 16 n .. b0 + 16 n + 15); in the band when a pair of it is
    bool live[LD_NT];
    bool any = false;
#pragma unroll
    for (int n = 0; n < LD_NT; ++n) {
        const int bc = b0 + n * 16;
        live[n] = bc + 15 > aw && bc <= aw + 15 + A.window && bc + 15 >= A.b_begin && bc < A.n_variants && aw < A.n_variants;
        any = any || live[n];
    }

    auto a_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + kq;
        if (any && a_ok && c < A.chunks) return load16o<false>(arow, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);                             // all missing: contributes nothing
    };
    auto b_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + sc;
        if (b_ok && c < A.chunks) return load16o<false>(brow, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);
    };
    auto stage = [&](int buf, const uint4 &raw) {
        uint4 v, g, q;
        ld_planes(raw.x, v.x, g.x, q.x);
        ld_planes(raw.y, v.y, g.y, q.y);
        ld_planes(raw.z, v.z, g.z, q.z);
        ld_planes(raw.w, v.w, g.w, q.w);
        bt[buf][0][sr * LD_LDS_ROW + sc] = v;
        bt[buf][1][sr * LD_LDS_ROW + sc] = g;
        bt[buf][2][sr * LD_LDS_ROW + sc] = q;
    };

    // per block the sums in counts6 order: n, sa, sb, saa, sbb, sab
    perm_i32x4 acc[LD_NT][6];
#pragma unroll
    for (int n = 0; n < LD_NT; ++n)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[n][k] = perm_i32x4{0, 0, 0, 0};

    stage(0, b_chunk(0));
    uint4 ga = a_chunk(0);
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        uint4 gan = make_uint4(~0u, ~0u, ~0u, ~0u), gbn = gan;
        if (more) { gan = a_chunk(s + 1); gbn = b_chunk(s + 1); }
        if (any) {
            perm_i32x4 av, ag, aq;
            {
                uint32_t v, g, q;
                ld_planes(ga.x, v, g, q); av[0] = (int)v; ag[0] = (int)g; aq[0] = (int)q;
                ld_planes(ga.y, v, g, q); av[1] = (int)v; ag[1] = (int)g; aq[1] = (int)q;
                ld_planes(ga.z, v, g, q); av[2] = (int)v; ag[2] = (int)g; aq[2] = (int)q;
                ld_planes(ga.w, v, g, q); av[3] = (int)v; ag[3] = (int)g; aq[3] = (int)q;
            }
            const int cur = s & 1;
#pragma unroll
            for (int n = 0; n < LD_NT; ++n) {
                if (!live[n]) continue;
                const int at = (n * 16 + col) * LD_LDS_ROW + kq;
                const uint4 pv = bt[cur][0][at], pg = bt[cur][1][at], pq = bt[cur][2][at];
                const perm_i32x4 bv = {(int)pv.x, (int)pv.y, (int)pv.z, (int)pv.w};
                const perm_i32x4 bg = {(int)pg.x, (int)pg.y, (int)pg.z, (int)pg.w};
                const perm_i32x4 bq = {(int)pq.x, (int)pq.y, (int)pq.z, (int)pq.w};
                acc[n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc[n][0], 0, 0, 0);
                acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bv, acc[n][1], 0, 0, 0);
                acc[n][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bg, acc[n][2], 0, 0, 0);
                acc[n][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aq, bv, acc[n][3], 0, 0, 0);
                acc[n][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bq, acc[n][4], 0, 0, 0);
                acc[n][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bg, acc[n][5], 0, 0, 0);
            }
        }
        if (more) stage((s + 1) & 1, gbn);
        __syncthreads();
        ga = gan;
    }

    // ---- epilogue: acc[n][k][r] belongs to the pair (a, b) = (aw + 4 kq + r, b0 + 16 n + col)
    const bool filter = A.chrom != nullptr;
#pragma unroll
    for (int n = 0; n < LD_NT; ++n) {
        if (!live[n]) continue;
        const int b = b0 + n * 16 + col;
        if (b < A.b_begin || b >= A.n_variants) continue;
        const bool b_skip = A.skip != nullptr && A.skip[b] != 0;
        const int b_chrom = filter ? A.chrom[b] : 0;
        const long long b_pos = filter ? (long long)A.pos[b] : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = aw + kq * 4 + r, d = b - a;
            if (d < 1 || d > A.window) continue;
            bool out = b_skip || (A.skip != nullptr && A.skip[a] != 0);
            if (filter && !out) {
                const long long dist = b_pos - (long long)A.pos[a];
                out = A.chrom[a] != b_chrom || (A.max_bp >= 0 && (dist < 0 ? -dist : dist) > A.max_bp);
            }
            const size_t at = (size_t)(b - A.b_begin) * (size_t)A.window + (size_t)(d - 1);
            int c[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) c[k] = out ? 0 : acc[n][k][r];
            A.r2[at] = out ? ld_nan() : ld_r2_value(c[0], c[1], c[2], c[3], c[4], c[5]);
            if (A.counts6 != nullptr) {
                int2 *o = reinterpret_cast<int2 *>(A.counts6 + at * 6);
                o[0] = make_int2(c[0], c[1]); o[1] = make_int2(c[2], c[3]); o[2] = make_int2(c[4], c[5]);
            }
        }
    }
}

// The edge form (hpgv_ld_edges_dev): k_ld_window's tile, lane maps, staging and skip logic, word for word, with another epilogue.
// It is a kernel of its own and not a compile-time form of one body, because k_ld_window's instructions are to stay what they
// were: with the body shared through a template the compiler allocated the band form's registers differently.  A change to
// the loop of one of the two belongs in the other.
//
// what the edge form writes instead of the band: the pairs with r2 >= min_r2 as records of 16 bytes
struct LdEdgeOut {
    double min_r2;                   // not NaN
    uint4 *edges;                    // {a, b, r2 low word, r2 high word} per record: hpgv_ld_edge; may be null when cap is 0
    unsigned long long cap;          // records behind `edges`: nothing is stored past them
    unsigned long long *n_edges;     // zeroed before the launch; ends as the number of qualifying pairs, stored or not
};

__global__ __launch_bounds__(256) void k_ld_edges(const LdArgs A, const LdEdgeOut E) {
    __shared__ uint4 bt[2][3][LD_BT * LD_LDS_ROW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    // workgroup -> (tile, pass), see "Grid" above
    const int range = (int)(blockIdx.x & 7u);
    const unsigned seq = blockIdx.x >> 3;
    const int in_range = (int)(seq / (unsigned)A.passes), pass = (int)(seq % (unsigned)A.passes);
    const int tile = range * A.tiles_per_range + in_range;
    if (in_range >= A.tiles_per_range || tile >= A.tiles) return;          // (the whole workgroup)
    const int a0 = tile * LD_VT, b0 = a0 + pass * LD_BT;
    // nothing to write: the group lies past the last row or wholly below b_begin
    if (b0 >= A.n_variants || b0 + LD_BT <= A.b_begin) return;

    const int aw = a0 + wave * 16;                                         // the wave's 16 earlier variants
    const int a_lane = aw + col;
    const bool a_ok = a_lane < A.n_variants;
    const uint8_t *arow = A.gt + (size_t)(a_ok ? a_lane : 0) * A.pitch;
    const int steps = (A.chunks + 3) / 4;
    // the chunk of the later rows this thread stages: row tid >> 2 of the group, chunk tid & 3 of the k-step
    const int sr = tid >> 2, sc = tid & 3;
    const bool b_ok = b0 + sr < A.n_variants;
    const uint8_t *brow = A.gt + (size_t)(b_ok ? b0 + sr : 0) * A.pitch;

    // block n of the wave holds the pairs (aw .. aw + 15) x (b0 + 16 n .. b0 + 16 n + 15); in the band when a pair of it is
    bool live[LD_NT];
    bool any = false;
#pragma unroll
    for (int n = 0; n < LD_NT; ++n) {
        const int bc = b0 + n * 16;
        live[n] = bc + 15 > aw && bc <= aw + 15 + A.window && bc + 15 >= A.b_begin && bc < A.n_variants && aw < A.n_variants;
        any = any || live[n];
    }

    auto a_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + kq;
        if (any && a_ok && c < A.chunks) return load16o<false>(arow, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);                             // all missing: contributes nothing
    };
    auto b_chunk = [&](int s) -> uint4 {
        const int c = s * 4 + sc;
        if (b_ok && c < A.chunks) return load16o<false>(brow, (uint32_t)c * 16u);
        return make_uint4(~0u, ~0u, ~0u, ~0u);
    };
    auto stage = [&](int buf, const uint4 &raw) {
        uint4 v, g, q;
        ld_planes(raw.x, v.x, g.x, q.x);
        ld_planes(raw.y, v.y, g.y, q.y);
        ld_planes(raw.z, v.z, g.z, q.z);
        ld_planes(raw.w, v.w, g.w, q.w);
        bt[buf][0][sr * LD_LDS_ROW + sc] = v;
        bt[buf][1][sr * LD_LDS_ROW + sc] = g;
        bt[buf][2][sr * LD_LDS_ROW + sc] = q;
    };

    // per block the sums in counts6 order: n, sa, sb, saa, sbb, sab
    perm_i32x4 acc[LD_NT][6];
#pragma unroll
    for (int n = 0; n < LD_NT; ++n)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[n][k] = perm_i32x4{0, 0, 0, 0};

    stage(0, b_chunk(0));
    uint4 ga = a_chunk(0);
    __syncthreads();

    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        uint4 gan = make_uint4(~0u, ~0u, ~0u, ~0u), gbn = gan;
        if (more) { gan = a_chunk(s + 1); gbn = b_chunk(s + 1); }
        if (any) {
            perm_i32x4 av, ag, aq;
            {
                uint32_t v, g, q;
                ld_planes(ga.x, v, g, q); av[0] = (int)v; ag[0] = (int)g; aq[0] = (int)q;
                ld_planes(ga.y, v, g, q); av[1] = (int)v; ag[1] = (int)g; aq[1] = (int)q;
                ld_planes(ga.z, v, g, q); av[2] = (int)v; ag[2] = (int)g; aq[2] = (int)q;
                ld_planes(ga.w, v, g, q); av[3] = (int)v; ag[3] = (int)g; aq[3] = (int)q;
            }
            const int cur = s & 1;
#pragma unroll
            for (int n = 0; n < LD_NT; ++n) {
                if (!live[n]) continue;
                const int at = (n * 16 + col) * LD_LDS_ROW + kq;
                const uint4 pv = bt[cur][0][at], pg = bt[cur][1][at], pq = bt[cur][2][at];
                const perm_i32x4 bv = {(int)pv.x, (int)pv.y, (int)pv.z, (int)pv.w};
                const perm_i32x4 bg = {(int)pg.x, (int)pg.y, (int)pg.z, (int)pg.w};
                const perm_i32x4 bq = {(int)pq.x, (int)pq.y, (int)pq.z, (int)pq.w};
                acc[n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc[n][0], 0, 0, 0);
                acc[n][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bv, acc[n][1], 0, 0, 0);
                acc[n][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bg, acc[n][2], 0, 0, 0);
                acc[n][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aq, bv, acc[n][3], 0, 0, 0);
                acc[n][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bq, acc[n][4], 0, 0, 0);
                acc[n][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag, bg, acc[n][5], 0, 0, 0);
            }
        }
        if (more) stage((s + 1) & 1, gbn);
        __syncthreads();
        ga = gan;
    }

    // ---- epilogue: acc[n][k][r] belongs to the pair (a, b) = (aw + 4 kq + r, b0 + 16 n + col)
    const bool filter = A.chrom != nullptr;
    // The edge form: the same r2 per pair (NaN where the band form writes NaN or nothing: NaN >= x is false), then per
    // (block, register) the wave's qualifying lanes by ballot, ONE 64-bit add of their number for the wave, and each such
    // lane's record at the returned base + its rank among them, one 16-byte store, when that index is below `cap`.  live[n]
    // is the same for every lane of the wave, so every lane reaches the ballot.
#pragma unroll
    for (int n = 0; n < LD_NT; ++n) {
        if (!live[n]) continue;
        const int b = b0 + n * 16 + col;
        const bool b_in = b >= A.b_begin && b < A.n_variants;
        const bool b_skip = b_in && A.skip != nullptr && A.skip[b] != 0;
        const int b_chrom = (b_in && filter) ? A.chrom[b] : 0;
        const long long b_pos = (b_in && filter) ? (long long)A.pos[b] : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = aw + kq * 4 + r, d = b - a;
            double v = ld_nan();
            if (b_in && d >= 1 && d <= A.window) {                     // (so 0 <= a < b < n_variants)
                bool out = b_skip || (A.skip != nullptr && A.skip[a] != 0);
                if (filter && !out) {
                    const long long dist = b_pos - (long long)A.pos[a];
                    out = A.chrom[a] != b_chrom || (A.max_bp >= 0 && (dist < 0 ? -dist : dist) > A.max_bp);
                }
                if (!out) v = ld_r2_value(acc[n][0][r], acc[n][1][r], acc[n][2][r], acc[n][3][r], acc[n][4][r], acc[n][5][r]);
            }
            const bool hit = v >= E.min_r2;
            const unsigned long long mask = __ballot(hit);
            if (mask == 0) continue;                                   // (the whole wave)
            const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
            unsigned long long base = 0;
            if (lane == leader)
                base = __hip_atomic_fetch_add(E.n_edges, (unsigned long long)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)base, leader);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(base >> 32), leader);
            const unsigned long long rank = (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            const unsigned long long at = (((unsigned long long)hi << 32) | lo) + rank;
            if (hit && at < E.cap) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
                E.edges[at] = make_uint4((unsigned)a, (unsigned)b, (unsigned)bits, (unsigned)(bits >> 32));
            }
        }
    }
}

}  // namespace hpgv
