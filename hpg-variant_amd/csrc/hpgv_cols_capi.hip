// hpgv_cols_capi.hip -- the host side that the tools over sample COLUMNS share (hpgv_ibs_capi.hip, hpgv_grm_capi.hip,
// hpgv_score_capi.hip; declared in hpgv_internal.h): the checks of a device matrix, the grid of a launch (hpgv_cols_kernels.h
// "Grid"), the class counts per row with their kernels, and the front and back of the synchronous entry points' back halves.
#include "hpgv_internal.h"
#include "hpgv_cols_kernels.h"

namespace hpgv {

// {n0, n1, n2, missing} of every row over the columns below n_cols, one wave per row; a skipped row gets zeros.  No scan of the
// engine yields these for a matrix without a cohort: the stats counters split the calls by allele pair (a "1/2" is in none of
// their four cells) and the model scan's classes are per phenotype group of the assoc layout.
static __global__ __launch_bounds__(256) void k_cols_class_counts(const uint8_t *__restrict__ gt, size_t pitch, int n_variants, int n_cols,
                                                                  const uint8_t *__restrict__ skip, int4 *__restrict__ class4) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_variants) return;                                         // (the whole wave)
    const bool out = skip != nullptr && skip[row] != 0;
    int n1 = 0, n2 = 0, nv = 0;
    if (!out) {
        const uint8_t *r = gt + (size_t)row * pitch;
        const int chunks = (n_cols + 15) / 16;
        for (int c = lane; c < chunks; c += 64) {
            const uint4 q = load16o<false>(r, (uint32_t)c * 16u);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int left = n_cols - (c * 16 + k * 4);                // columns of this dword below n_cols
                const uint32_t x = left >= 4 ? w[k] : (left <= 0 ? ~0u : (w[k] | (~0u << (8 * left))));
                uint32_t v, g;
                perm_planes_trend(x, v, g);
                nv += __builtin_popcount(v);
                n1 += __builtin_popcount(g & 0x01010101u);
                n2 += __builtin_popcount(g & 0x02020202u);
            }
        }
    }
    nv = wave_sum(nv); n1 = wave_sum(n1); n2 = wave_sum(n2);
    if (lane == 0) class4[row] = out ? make_int4(0, 0, 0, 0) : make_int4(nv - n1 - n2, n1, n2, n_cols - nv);
}

// skip[k] |= is_x[k]: the text form's rule for chromosome X
static __global__ __launch_bounds__(256) void k_cols_skip_x(uint8_t *__restrict__ skip, const uint8_t *__restrict__ is_x, int n) {
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k < n && is_x[k] != 0) skip[k] = 1;
}

}  // namespace hpgv

int cols_matrix_check(const hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols) {
    if (n_variants < 0 || n_cols < 0 || (size_t)n_cols > pitch) return fail(ctx, HPGV_ERR_INVALID, "bad matrix arguments: %d rows, %d columns, pitch %zu", n_variants, n_cols, pitch);
    if (pitch == 0 || (pitch & 15) || pitch > 0xFFFFFFF0u) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu: a multiple of 16 below 4 GiB", pitch);
    if ((uintptr_t)d_gt & 15) return fail(ctx, HPGV_ERR_INVALID, "d_gt must be 16-byte aligned");
    return HPGV_OK;
}

int cols_grid_fill(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, long long work, int rows, const char *what,
                   hpgv::ColsGrid *G) {
    G->gt = d_gt; G->pitch = pitch; G->n_variants = n_variants; G->n_cols = n_cols; G->skip = d_skip;
    G->work = work;
    G->rows_per_split = rows;
    G->splits = (int)(((long long)n_variants + rows - 1) / rows);
    G->items = (unsigned long long)work * (unsigned long long)G->splits;
    const unsigned long long per_xcd = (G->items + 7) / 8;
    if (per_xcd * 8 > 0x7FFFFFFFull)
        return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d columns, %d rows: %lld %s in %d row ranges exceed the grid", n_cols, n_variants, work, what, G->splits);
    G->per_xcd = (unsigned)per_xcd;
    return HPGV_OK;
}

int cols_class_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, int32_t *d_class4, hipStream_t st) {
    hipLaunchKernelGGL(hpgv::k_cols_class_counts, dim3((unsigned)(((long long)n_variants + 3) / 4)), dim3(256), 0, st, d_gt, pitch, n_variants, n_cols, d_skip,
                       reinterpret_cast<int4 *>(d_class4));
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

// The STATS layout holds every sample in VCF order, but its bytes are the stats flags and not HPGV8: the kernels read the RAW
// matrix, which has the same columns -- in place where its pitch is a multiple of 16 (a text's always is), else gathered into the
// slot's `laid` in the stats layout's pitch without recoding.
int cols_front(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, bool need_skip, ColsFront *F) {
    const int nv = S.n, ns = ctx->stats.n_samples;
    const size_t n = (size_t)nv;
    const uint8_t *d_gt = S.d_raw;
    size_t gt_pitch = S.raw_pitch;
    if ((gt_pitch & 15) || ((uintptr_t)d_gt & 15)) {
        const Layout &L = ctx->stats;
        HIPCHK(ctx, s->laid.reserve_slack(n * L.pitch + 16));
        const long slab = std::max(1L, (1L << 31) / (L.chunks > 0 ? L.chunks : 1));      // (hpgv_layout_dev's launches)
        for (long off = 0; off < nv; off += slab) {
            const int m = (int)std::min(slab, (long)nv - off);
            hipLaunchKernelGGL(hpgv::k_layout, dim3((unsigned)(((long)m * L.chunks + 255) / 256)), dim3(256), 0, s->stream,
                               S.d_raw + (size_t)off * S.raw_pitch, S.raw_pitch, m, L.pitch, L.chunks, L.d_col_of_pos(), 0, (int)hpgv::RECODE_NONE, 0,
                               s->laid.as<uint8_t>() + (size_t)off * L.pitch);
        }
        HIPCHK(ctx, hipGetLastError());
        d_gt = s->laid.as<uint8_t>(); gt_pitch = L.pitch;
    }
    const bool have_skip = skip != nullptr || x_too || need_skip;
    HIPCHK(ctx, s->tally.reserve_slack(n * 16 + 16));
    if (have_skip) HIPCHK(ctx, s->perm.reserve_slack(n + 16));
    int32_t *d_class4 = s->tally.as<int32_t>();
    uint8_t *d_skip = have_skip ? s->perm.as<uint8_t>() : nullptr;
    if (skip) HIPCHK(ctx, hipMemcpyAsync(d_skip, skip, n, hipMemcpyHostToDevice, s->stream));
    else if (have_skip) HIPCHK(ctx, hipMemsetAsync(d_skip, 0, n, s->stream));
    if (x_too) {
        hipLaunchKernelGGL(hpgv::k_cols_skip_x, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s->stream, d_skip, S.d_isx, nv);
        HIPCHK(ctx, hipGetLastError());
    }
    if (const int rc = cols_class_launch(ctx, d_gt, gt_pitch, nv, ns, d_skip, d_class4, s->stream)) return rc;
    F->d_gt = d_gt; F->pitch = gt_pitch; F->d_skip = d_skip; F->d_class4 = d_class4;
    return HPGV_OK;
}

int cols_back(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, bool need_skip, int32_t *class4, const std::function<int(const ColsFront &)> &body) {
    if (S.n > 0) {
        ColsFront F;
        if (const int rc = cols_front(ctx, s, S, skip, x_too, need_skip, &F)) return rc;
        if (const int rc = body(F)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(class4, F.d_class4, (size_t)S.n * 16, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}
