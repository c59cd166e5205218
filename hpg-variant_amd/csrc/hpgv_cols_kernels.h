// hpgv_cols_kernels.h -- what the kernels that contract over the ROWS of one genotype matrix, between or per its sample COLUMNS,
// share (gfx950): the tile and its LDS image, the 4 x 4 byte transposition, the grid over (row range, work unit) with its
// row-range plan, and the walk of one tile pair that k_ibs_pairs (hpgv_ibs_kernels.h) and k_grm_pairs (hpgv_grm_kernels.h) are.
// k_score_cols (hpgv_score_kernels.h) has one side and a loop of its own and takes the grid, the staging address and the fragment
// read from here.
//
// Transposition.  K runs over the ROWS of the matrix, and an operand fragment is 16 consecutive-k bytes of ONE column.  Per
// k-step of 64 rows a thread loads four dwords: the same four columns of four consecutive rows.  Two rounds of v_perm_b32 turn
// them into four dwords that each hold four consecutive k of one column.  Where the plane code is bytewise SWAR (IBS, score) the
// RAW bytes are transposed and the planes formed afterwards: it commutes with the permutation, which is then paid once and not
// per plane.
//
// Lane maps.  A and B: lane l holds column l & 15 of its block and the 16 k values of lane group l >> 4.  In the pair walk BOTH
// operands are read from the LDS image through the same path at the same k -- the A fragment of a column is the very b128 a B
// fragment of that column would be -- so the sums do not depend on how the hardware numbers the k values inside a lane group, nor
// on the order in which v_perm_b32 leaves the four k of a dword.  C/D: col = l & 15 (column j), row = (l >> 4) * 4 + reg (column i).
//
// Tile.  A workgroup of four waves owns COLS_T = 64 columns I (16 per wave) x 64 columns J >= I and a range of rows.  The k-step's
// two 64 x 64 byte blocks are staged in LDS AS PLANES, transposed: 2 sides x NP planes x 64 columns x 64 bytes, columns 80 bytes
// apart (bank spread of the b128 reads), two buffers, one barrier per k-step.  Staging raw bytes would make each of the four waves
// form the planes of all 64 J columns again after its reads: 4 times the vector work, and the vector ALU, not the matrix pipe,
// bounds these kernels (DESIGN "IBS pairs").  A diagonal tile stages one side and reads both operands from it, and computes the
// blocks on and above the diagonal.  A block whose columns all lie at or past n_cols issues nothing; columns at or past n_cols
// and rows that are skipped or past the range load as 0xFF.
//
// Grid.  One-dimensional over (row range, work unit), the unit -- a tile pair, or a tile -- fastest.  Workgroups are dealt to the
// 8 XCDs in turn (w % 8) and an XCD's L2 is not shared, so the items are cut into 8 contiguous runs, one per value of w % 8: the
// workgroups in flight on one XCD work on the same row range and on neighbouring tile pairs, which share their J tile.  A matter
// of speed alone (numbering the pairs in super-tiles of 8 x 8 tiles, so that 64 neighbours share 8 + 8 column tiles, measured no
// faster: DESIGN "IBS pairs").  The row ranges exist because few columns give few tiles (200 samples: 10 pairs on 256 CUs).
#pragma once
#include "hpgv_assoc_perm_kernels.h"
#include <math.h>

namespace hpgv {

constexpr int COLS_T = 64;            // columns per tile side: 16 per wave on the I side
constexpr int COLS_NT = COLS_T / 16;
constexpr int COLS_LDS_COL = 5;       // uint4 per staged column: 64 k bytes + 16 of padding
constexpr int COLS_SPLIT_ROWS = 256;  // a row range is never shorter than this (but for the last)

// column tiles, and tile pairs (ti <= tj), of n_cols columns; at least one
inline long long cols_tiles(int n_cols) { return ((long long)(n_cols > 0 ? n_cols : 1) + COLS_T - 1) / COLS_T; }
inline long long cols_tile_pairs(int n_cols) { return cols_tiles(n_cols) * (cols_tiles(n_cols) + 1) / 2; }

// Rows per row range: the ranges fill the device about `depth` workgroups per CU deep where the `work` units alone do not, none
// shorter than COLS_SPLIT_ROWS rows, with at least as many ranges as `cap` (a multiple of 64) asks for.  A multiple of 64, at
// least 64, at most the cap
inline int cols_plan_rows(int n_variants, long long work, int depth, long long cap, int n_cus) {
    const long long nv = n_variants > 0 ? n_variants : 0;
    const long long want = ((long long)depth * (n_cus > 0 ? n_cus : 1) + work - 1) / work, room = (nv + COLS_SPLIT_ROWS - 1) / COLS_SPLIT_ROWS;
    long long splits = want < room ? (want > 1 ? want : 1) : (room > 1 ? room : 1);
    const long long least = (nv + cap - 1) / cap;
    if (splits < least) splits = least;
    // EQUAL ranges, not ranges of the cap and a rest: the grid deals contiguous runs of (range, unit) items to the XCDs, and a short
    // last range would leave the XCDs that draw it idle (measured on k_grm_pairs: 10 000 x 32 832 as 32 768 + 64 rows took twice
    // the time of one range)
    const long long rows = ((nv + splits - 1) / splits + 63) / 64 * 64;             // <= the cap: the cap is a multiple of 64
    return (int)(rows < 64 ? 64 : rows);
}

// the matrix and the grid of a launch (cols_grid_fill, hpgv_cols_capi.hip)
struct ColsGrid {
    const uint8_t *gt;               // rows of HPGV8 bytes `pitch` apart
    size_t pitch;
    int n_variants, n_cols;
    const uint8_t *skip;             // per row, may be null
    long long work;                  // units per row range: tile pairs, tiles (tiles + 1) / 2 with tiles = ceil(n_cols / COLS_T), or tiles
    int splits, rows_per_split;      // row ranges; rows of each, a multiple of 64
    unsigned long long items;        // work * splits
    unsigned per_xcd;                // ceil(items / 8): the grid is 8 per_xcd workgroups
};

// a workgroup's item: its unit within `work`, its rows k_begin .. k_end - 1 in `steps` k-steps of 64
struct ColsItem {
    long long unit;
    int k_begin, k_end, steps;
};

// steps == 0: the workgroup (the whole of it) has nothing to do
__device__ __forceinline__ ColsItem cols_item(const ColsGrid &G) {
    ColsItem it{0, 0, 0, 0};
    const unsigned seq = blockIdx.x >> 3;
    const unsigned long long item = (unsigned long long)(blockIdx.x & 7u) * G.per_xcd + seq;
    if (seq >= G.per_xcd || item >= G.items) return it;
    const int split = (int)(item / (unsigned long long)G.work);
    const long long k_first = (long long)split * G.rows_per_split;
    if (k_first >= G.n_variants) return it;
    it.unit = (long long)(item % (unsigned long long)G.work);
    it.k_begin = (int)k_first;
    it.k_end = (int)min((long long)G.n_variants, k_first + G.rows_per_split);
    it.steps = (it.k_end - it.k_begin + 63) / 64;
    return it;
}

// the 4 x 4 byte transpose: r[k] holds the bytes of columns c .. c + 3 in row k; afterwards r[c] holds the four rows of column c
__device__ __forceinline__ void cols_transpose4(uint32_t (&r)[4]) {
    const uint32_t a = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u);   // columns 0, 0, 1, 1 of rows 0 and 1
    const uint32_t b = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);   // columns 2, 2, 3, 3
    const uint32_t c = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u);   // the same of rows 2 and 3
    const uint32_t d = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
    r[0] = __builtin_amdgcn_perm(c, a, 0x05040100u);
    r[1] = __builtin_amdgcn_perm(c, a, 0x07060302u);
    r[2] = __builtin_amdgcn_perm(d, b, 0x05040100u);
    r[3] = __builtin_amdgcn_perm(d, b, 0x07060302u);
}

// One plane of one side of the LDS image is COLS_T * COLS_LDS_COL uint4.  Thread (cg, rg) = (tid & 15, tid >> 4) stages rows
// 4 rg .. 4 rg + 3 of columns 4 cg .. 4 cg + 3: the dword of column 4 cg + c; lane (col, kq) reads 16 k of column `column`
__device__ __forceinline__ uint32_t &cols_staged(uint4 *plane, int cg, int c, int rg) {
    return reinterpret_cast<uint32_t *>(plane)[(4 * cg + c) * (COLS_LDS_COL * 4) + rg];
}
__device__ __forceinline__ perm_i32x4 cols_frag(const uint4 *plane, int column, int kq) {
    const uint4 q = plane[column * COLS_LDS_COL + kq];
    return perm_i32x4{(int)q.x, (int)q.y, (int)q.z, (int)q.w};
}

__device__ __forceinline__ long long cols_wave_sum_i64(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The walk of one (row range, tile pair) item by a workgroup of 256 threads: four sums per pair of columns, acc[n][0 .. 3].
// What a tool is, is its Op:
//     NP                      planes staged per side
//     DIAG                    whether the pairs i == j are written (i < j always are)
//     Row, row(k, ok)         what a thread holds per fetched row beside the genotypes (ok: the row is in the range and not skipped)
//     planes(r, t, pl)        the raw dwords r[4] (four columns of four rows; may be clobbered) with their rows' t[4] -> pl[q][c]:
//                             plane q of column c, its four rows in one dword
//     mma(a, b, acc)          the MFMAs of one block on the fragments a[NP] of the I columns and b[NP] of the J columns
//     emit(i, j, n_cols, ..)  adds the four sums of the pair (i, j)
template <class Op>
__device__ __forceinline__ void cols_pair_walk(const ColsGrid &G, const Op &op, uint4 (&img)[2][2][Op::NP][COLS_T * COLS_LDS_COL]) {
    constexpr int NP = Op::NP;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, kq = lane >> 4;
    const ColsItem it = cols_item(G);
    if (it.steps == 0) return;
    // unit p = tj (tj + 1) / 2 + ti with ti <= tj
    const long long p = it.unit;
    long long tj = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((tj + 1) * (tj + 2) / 2 <= p) ++tj;
    while (tj * (tj + 1) / 2 > p) --tj;
    const int ti = (int)(p - tj * (tj + 1) / 2);
    const bool diag = ti == (int)tj;
    const int i0 = ti * COLS_T, j0 = (int)tj * COLS_T;
    const int k_begin = it.k_begin, k_end = it.k_end, steps = it.steps;

    // what this thread stages: columns 4 cg .. 4 cg + 3 of each side, rows 4 rg .. 4 rg + 3 of the k-step
    const int cg = tid & 15, rg = tid >> 4;
    const int ci = i0 + 4 * cg, cj = j0 + 4 * cg;
    const bool ci_ok = ci < G.n_cols, cj_ok = !diag && cj < G.n_cols;      // (ci + 4 <= pitch then: a multiple of 16 >= n_cols)

    // block n of the wave holds the pairs (iw .. iw + 15) x (j0 + 16 n .. j0 + 16 n + 15)
    const int iw = i0 + wave * 16;
    bool live[COLS_NT];
    bool any = false;
#pragma unroll
    for (int n = 0; n < COLS_NT; ++n) {
        live[n] = iw < G.n_cols && j0 + n * 16 < G.n_cols && (!diag || n >= wave);
        any = any || live[n];
    }

    auto fetch = [&](int s, uint32_t (&ra)[4], uint32_t (&rb)[4], typename Op::Row (&t)[4]) {
        const int kb = k_begin + s * 64 + 4 * rg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kb + r;
            const bool ok = k < k_end && (G.skip == nullptr || G.skip[k] == 0);
            const uint8_t *row = G.gt + (size_t)(ok ? k : 0) * G.pitch;
            t[r] = op.row(k, ok);
            ra[r] = (ok && ci_ok) ? *reinterpret_cast<const uint32_t *>(row + ci) : ~0u;
            rb[r] = (ok && cj_ok) ? *reinterpret_cast<const uint32_t *>(row + cj) : ~0u;
        }
    };
    auto stage_side = [&](int buf, int side, uint32_t (&r)[4], const typename Op::Row (&t)[4]) {
        uint32_t pl[NP][4];
        op.planes(r, t, pl);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < NP; ++q) cols_staged(img[buf][side][q], cg, c, rg) = pl[q][c];
    };
    auto stage = [&](int buf, uint32_t (&ra)[4], uint32_t (&rb)[4], const typename Op::Row (&t)[4]) {
        stage_side(buf, 0, ra, t);
        if (!diag) stage_side(buf, 1, rb, t);
    };
    auto frags = [&](int buf, int side, int column, perm_i32x4 (&f)[NP]) {
#pragma unroll
        for (int q = 0; q < NP; ++q) f[q] = cols_frag(img[buf][side][q], column, kq);
    };

    perm_i32x4 acc[COLS_NT][4];
#pragma unroll
    for (int n = 0; n < COLS_NT; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[n][k] = perm_i32x4{0, 0, 0, 0};

    uint32_t ra[4], rb[4];
    typename Op::Row tb[4];
    fetch(0, ra, rb, tb);
    stage(0, ra, rb, tb);
    __syncthreads();

    const int bside = diag ? 0 : 1;
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) fetch(s + 1, ra, rb, tb);
        if (any) {
            const int cur = s & 1;
            perm_i32x4 a[NP];
            frags(cur, 0, wave * 16 + col, a);
#pragma unroll
            for (int n = 0; n < COLS_NT; ++n) {
                if (!live[n]) continue;
                perm_i32x4 b[NP];
                frags(cur, bside, n * 16 + col, b);
                Op::mma(a, b, acc[n]);
            }
        }
        if (more) stage((s + 1) & 1, ra, rb, tb);
        __syncthreads();
    }

    // ---- epilogue: acc[n][k][r] belongs to the pair (i, j) = (iw + 4 kq + r, j0 + 16 n + col)
#pragma unroll
    for (int n = 0; n < COLS_NT; ++n) {
        if (!live[n]) continue;
        const int j = j0 + n * 16 + col;
        if (j >= G.n_cols) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = iw + kq * 4 + r;
            if (i > j || (!Op::DIAG && i == j)) continue;
            op.emit(i, j, G.n_cols, acc[n][0][r], acc[n][1][r], acc[n][2][r], acc[n][3][r]);
        }
    }
}

}  // namespace hpgv
