// hpgv_perm_capi.hip -- C ABI of the max(T) permutations (include/hpgv.h "label permutation", "family flips"): the label rows
// of the association test and the flip rows of the TDT of a context, the device-resident launches of k_assoc_perm and
// k_tdt_perm, the synchronous entry points on a host batch and on a text, and the host-only helpers (label shuffle, flip
// generator, empirical p-values).  The genotypic model tests (include/hpgv.h "model tests") live here too: their class scan and
// statistics kernels, and the trend form of k_assoc_perm behind the same launcher as the allelic one.
// A synchronous entry point checks its arguments, leases a slot and stages like every tool's (stage_chain for a batch,
// text_front_skip for a text: hpgv_internal.h); its back half is the tool's own chain with the permutation launch between the
// chain's two halves (assoc_chain / assoc_copy_out, tdt_chain / tdt_copy_out: hpgv_tool_capi.hip) -- the model tests alone keep a
// chain of their own -- and perm_plan (hpgv_internal.h) lays out the call's scratch in Slot::perm.
#include "hpgv_internal.h"
#include "hpgv_assoc_model_kernels.h"
#include "hpgv_assoc_perm_kernels.h"
#include "hpgv_tdt_perm_kernels.h"

namespace {

static_assert(hpgv::MODEL_GENO == HPGV_MODEL_GENO && hpgv::MODEL_TREND == HPGV_MODEL_TREND && hpgv::MODEL_ALLELIC == HPGV_MODEL_ALLELIC &&
              hpgv::MODEL_DOM == HPGV_MODEL_DOM && hpgv::MODEL_REC == HPGV_MODEL_REC, "the kernels' test order is the header's");

constexpr int kMaxPerms = 1 << 20;     // PERM_PT permutations per workgroup row of the grid: far below the grid's 65 535 rows

int perm_state_check(const hpgv_ctx *ctx) {
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (ctx->n_perms <= 0) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_perm_labels has not been called (a new cohort drops the labels)");
    return HPGV_OK;
}

// the launch: n_ge and batch_max zeroed on the stream, then the kernel in its form (hpgv::PERM_ALLELIC: d_counts of
// hpgv_assoc_scan_dev; hpgv::PERM_TREND: the counts8 of hpgv_assoc_model_scan_dev, no d_is_x)
int perm_launch(hpgv_ctx *ctx, int form, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_counts, const uint8_t *d_skip,
                int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_counts, hipStream_t st) {
    HIPCHK(ctx, hipMemsetAsync(d_batch_max, 0, (size_t)ctx->n_perms * sizeof(double), st));
    if (n_variants == 0) return HPGV_OK;
    HIPCHK(ctx, hipMemsetAsync(d_n_ge, 0, (size_t)n_variants * sizeof(int32_t), st));
    hpgv::PermArgs A;
    A.gt = d_gt; A.pitch = ctx->assoc.pitch; A.chunks = ctx->assoc.chunks; A.n_variants = n_variants;
    A.is_x = d_is_x; A.counts = (const int4 *)d_counts;
    A.labels = ctx->d_perm.as<uint8_t>(); A.n_perms = ctx->n_perms; A.label_rows = ctx->perm_rows;
    A.skip = d_skip; A.n_ge = d_n_ge; A.batch_max = (unsigned long long *)d_batch_max; A.perm_counts = d_perm_counts;
    const dim3 grid((unsigned)((n_variants + hpgv::PERM_VT - 1) / hpgv::PERM_VT), (unsigned)((ctx->n_perms + hpgv::PERM_PT - 1) / hpgv::PERM_PT));
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
        if (form == hpgv::PERM_TREND) hipLaunchKernelGGL(hpgv::k_assoc_perm<hpgv::PERM_TREND>, grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL(hpgv::k_assoc_perm<hpgv::PERM_ALLELIC>, grid, dim3(256), 0, st, A);
    });
}

/* ---- model tests ---------------------------------------------------------------------------------------------------- */

// the class scan on `st`: k_assoc_scan_pipe's grid (variants_per_wave consecutive rows per wave, four waves per workgroup)
int model_scan_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_counts8, hipStream_t st) {
    const Layout &L = ctx->assoc;
    if (L.chunks > hpgv::MODEL_MAX_CHUNKS)
        return fail(ctx, HPGV_ERR_UNSUPPORTED, "rows of %d chunks: the class scan's packed 16-bit counters take at most %d", L.chunks, hpgv::MODEL_MAX_CHUNKS);
    const int vpw = (int)ctx->vpw;
    const long waves = ((long)n_variants + vpw - 1) / vpw;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    return launch_profiled(ctx, st, 0, [&] {
        if (ctx->nontemporal)
            hipLaunchKernelGGL((hpgv::k_assoc_model_scan<true, 4, 4>), dim3(blocks), dim3(256), 0, st, d_gt, L.pitch, n_variants, ctx->chunksA, L.chunks,
                               ctx->nA, ctx->nU, (int4 *)d_counts8, vpw);
        else
            hipLaunchKernelGGL((hpgv::k_assoc_model_scan<false, 4, 4>), dim3(blocks), dim3(256), 0, st, d_gt, L.pitch, n_variants, ctx->chunksA, L.chunks,
                               ctx->nA, ctx->nU, (int4 *)d_counts8, vpw);
    });
}

int model_stats_launch(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants, double *d_chisq5, double *d_p5, hipStream_t st) {
    return launch_profiled(ctx, st, 1, [&] {
        hipLaunchKernelGGL(hpgv::k_assoc_model_stats, dim3((unsigned)((n_variants + 255) / 256)), dim3(256), 0, st, (const int4 *)d_counts8, n_variants, d_chisq5, d_p5);
    });
}

// the back half of hpgv_assoc_model and hpgv_assoc_model_text: the laid-out matrix of a staged call -> class scan, the five
// statistics, with `perm` the trend form of the permutation kernel -> the caller's arrays.  skip (host, may be null): rows
// that take no part in the permutation
int model_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, bool perm, const uint8_t *skip, int32_t *counts8, double *chisq5, double *p5,
                 int32_t *n_ge, double *batch_max) {
    int rc;
    const int nv = S.n;
    const size_t n = (size_t)nv, np = perm ? (size_t)ctx->n_perms : 0;
    HIPCHK(ctx, s->tally.reserve_slack(n * 32 + 16));
    HIPCHK(ctx, s->dbl.reserve_slack(n * 10 * sizeof(double) + 16));
    PermPlan P;
    if (perm && (rc = perm_plan(ctx, s, n, np, skip, 0, &P))) return rc;
    int32_t *d_counts8 = s->tally.as<int32_t>();
    double *d_chisq5 = s->dbl.as<double>(), *d_p5 = d_chisq5 + 5 * n;
    if (nv > 0) {
        if ((rc = model_scan_launch(ctx, S.d_laid, nv, d_counts8, s->stream))) return rc;
        if ((rc = model_stats_launch(ctx, d_counts8, nv, d_chisq5, d_p5, s->stream))) return rc;
    }
    if (perm && (rc = perm_launch(ctx, hpgv::PERM_TREND, S.d_laid, nv, nullptr, d_counts8, P.d_skip, P.d_n_ge, P.d_max, nullptr, s->stream))) return rc;
    if (nv > 0) {
        HIPCHK(ctx, hipMemcpyAsync(counts8, d_counts8, n * 32, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(chisq5, d_chisq5, n * 40, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(p5, d_p5, n * 40, hipMemcpyDeviceToHost, s->stream));
        if (perm) HIPCHK(ctx, hipMemcpyAsync(n_ge, P.d_n_ge, n * 4, hipMemcpyDeviceToHost, s->stream));
    }
    if (perm) HIPCHK(ctx, hipMemcpyAsync(batch_max, P.d_max, np * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

// the back half of hpgv_assoc_perm and hpgv_assoc_perm_text: hpgv_assoc's kernel chain (task CHISQ) with the permutation kernel
// between its two halves.  On the slot's stream, in this order: the skip bytes (host, may be null: rows that take no part), scan,
// chi-square, the two memsets and k_assoc_perm, k_counts_to_soa, the copies out, one synchronise
int perm_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max) {
    int rc;
    const size_t n = (size_t)S.n, np = (size_t)ctx->n_perms;
    PermPlan P;
    ChainOut C;
    if ((rc = perm_plan(ctx, s, n, np, skip, 0, &P))) return rc;
    if ((rc = assoc_chain(ctx, s, HPGV_TASK_CHISQ, S, &C))) return rc;
    if ((rc = perm_launch(ctx, hpgv::PERM_ALLELIC, S.d_laid, S.n, S.d_isx, C.d_tally, P.d_skip, P.d_n_ge, P.d_max, nullptr, s->stream))) return rc;
    if ((rc = assoc_copy_out(ctx, s, HPGV_TASK_CHISQ, S, C, A1, A2, U1, U2, odds, chisq, p))) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(n_ge, P.d_n_ge, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(batch_max, P.d_max, np * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

/* ---- TDT, family flips ------------------------------------------------------------------------------------------- */

int flip_state_check(const hpgv_ctx *ctx) {
    if (!ctx->tdt.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_families has not been called");
    if (ctx->n_flips <= 0) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_tdt_flips has not been called (new families drop the flips)");
    return HPGV_OK;
}

int flip_tail_pitch(const hpgv_ctx *ctx) { return (int)round_up((size_t)ctx->tdt_plan.n_slow_families, 16); }

// the launch: n_ge and batch_max zeroed on the stream, the slow families' differences into d_tail (flip_tail_pitch bytes per
// row; unused without slow families), then the product kernel
int flip_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_tu, const uint8_t *d_skip,
                int8_t *d_tail, int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_tu, hipStream_t st) {
    HIPCHK(ctx, hipMemsetAsync(d_batch_max, 0, (size_t)ctx->n_flips * sizeof(double), st));
    if (n_variants == 0) return HPGV_OK;
    HIPCHK(ctx, hipMemsetAsync(d_n_ge, 0, (size_t)n_variants * sizeof(int32_t), st));
    const hpgv::TdtPlan &P = ctx->tdt_plan;
    const int tail_pitch = flip_tail_pitch(ctx);
    hpgv::TdtPermArgs A;
    A.gt = d_gt; A.pitch = ctx->tdt.pitch; A.pchunks = P.pchunks; A.kchunks = ctx->flip_pitch / 16; A.n_variants = n_variants;
    A.is_x = d_is_x; A.luts = P.luts; A.male_plane = P.d_male_plane;
    A.tail = tail_pitch ? d_tail : nullptr; A.tail_pitch = tail_pitch; A.tu = (const int2 *)d_tu;
    A.signs = ctx->d_flips.as<uint8_t>(); A.n_perms = ctx->n_flips; A.sign_rows = ctx->flip_rows;
    A.skip = d_skip; A.n_ge = d_n_ge; A.batch_max = (unsigned long long *)d_batch_max; A.perm_tu = d_perm_tu;
    // one workgroup per (variant tile, pass), the tiles rounded up to 8 (k_tdt_perm "Grid")
    A.passes = (ctx->n_flips + hpgv::PERM_PT - 1) / hpgv::PERM_PT;
    const size_t wgs = round_up((size_t)((n_variants + hpgv::PERM_VT - 1) / hpgv::PERM_VT), 8) * (size_t)A.passes;
    if (wgs > 0x7FFFFFFFu) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d variants x %d permutations in one call: give the variants in several", n_variants, ctx->n_flips);
    const dim3 grid((unsigned)wgs);
    // (option "profile": the two kernels' time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] {
        if (tail_pitch) {
            const size_t lanes = (size_t)n_variants * (size_t)tail_pitch;
            hipLaunchKernelGGL(hpgv::k_tdt_perm_slow, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, d_gt, ctx->tdt.pitch, n_variants,
                               P.n_slow_families, tail_pitch, P.d_slow_off, P.d_slow_male, P.slow_base, d_is_x, d_tail);
        }
        hipLaunchKernelGGL(hpgv::k_tdt_perm, grid, dim3(256), 0, st, A);
    });
}

// the back half of hpgv_tdt_perm and hpgv_tdt_perm_text: hpgv_tdt's kernel chain with the permutation kernels between its two
// halves.  On the slot's stream, in this order: the skip bytes (host, may be null: rows that take no part), scan, statistics, the
// two memsets, k_tdt_perm_slow and k_tdt_perm, the copies out, one synchronise
int flip_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p,
                int32_t *n_ge, double *batch_max) {
    int rc;
    const size_t n = (size_t)S.n, np = (size_t)ctx->n_flips;
    PermPlan P;
    ChainOut C;
    std::vector<int32_t> tu;
    if ((rc = perm_plan(ctx, s, n, np, skip, (size_t)flip_tail_pitch(ctx), &P))) return rc;
    if ((rc = tdt_chain(ctx, s, S, &C))) return rc;
    if ((rc = flip_launch(ctx, S.d_laid, S.n, S.d_isx, C.d_tally, P.d_skip, P.d_tail, P.d_n_ge, P.d_max, nullptr, s->stream))) return rc;
    if ((rc = tdt_copy_out(ctx, s, S, C, &tu, odds, chisq, p))) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(n_ge, P.d_n_ge, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(batch_max, P.d_max, np * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    tdt_split_counts(tu, t1, t2);
    return HPGV_OK;
}

// SplitMix64 (Steele, Lea, Flood 2014): the finalizer of the generator named in include/hpgv.h
inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

extern "C" {

int hpgv_set_perm_labels(hpgv_ctx *ctx, const uint8_t *labels, int n_perms) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_perm_labels(m_, labels, n_perms))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_perms < 0 || (n_perms > 0 && !labels)) return fail(ctx, HPGV_ERR_INVALID, "bad perm_labels arguments");
    if (n_perms > kMaxPerms) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d permutations: at most %d per call", n_perms, kMaxPerms);
    if (n_perms == 0) { ctx->n_perms = ctx->perm_rows = 0; return HPGV_OK; }
    const Layout &L = ctx->assoc;
    const size_t ns = (size_t)L.n_samples, rows = round_up((size_t)n_perms, 16);
    std::vector<uint8_t> laid(rows * L.pitch, 0);
    for (int q = 0; q < n_perms; ++q) {
        const uint8_t *src = labels + (size_t)q * ns;
        uint8_t *dst = laid.data() + (size_t)q * L.pitch;
        for (size_t pos = 0; pos < L.pitch; ++pos) {
            const int32_t j = L.col_of_pos[pos];
            if (j < 0) continue;
            if (src[j] > 1) return fail(ctx, HPGV_ERR_INVALID, "label %u of permutation %d, column %d: labels are 0 or 1", (unsigned)src[j], q, (int)j);
            dst[pos] = src[j];
        }
    }
    DeviceGuard g(ctx->device);
    ctx->n_perms = ctx->perm_rows = 0;
    {
        const hipError_t e = ctx->d_perm.reserve(laid.size());
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, HPGV_ERR_NOMEM, "the label matrix (%zu bytes) does not fit the device", laid.size()); }
        HIPCHK(ctx, e);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_perm.p, laid.data(), laid.size(), hipMemcpyHostToDevice));
    ctx->n_perms = n_perms; ctx->perm_rows = (int)rows;
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_counts,
                        int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_counts, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = perm_state_check(ctx)) return rc;
    if (n_variants < 0 || !d_batch_max || (n_variants > 0 && (!d_gt || !d_counts || !d_n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_perm arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_counts & 15) || ((uintptr_t)d_batch_max & 7) || ((uintptr_t)d_perm_counts & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_counts must be 16-byte aligned, d_batch_max and d_perm_counts 8-byte aligned");
    DeviceGuard g(ctx->device);
    return perm_launch(ctx, hpgv::PERM_ALLELIC, d_gt, n_variants, d_is_x, d_counts, nullptr, d_n_ge, d_batch_max, d_perm_counts, (hipStream_t)stream);
}

/* ---- model tests: class scan, the five statistics, trend permutation ------------------------------------------------ */

int hpgv_assoc_model_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_counts8, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_counts8))) return fail(ctx, HPGV_ERR_INVALID, "bad scan arguments");
    if (n_variants == 0) return HPGV_OK;
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_counts8 & 15)) return fail(ctx, HPGV_ERR_INVALID, "device buffers must be 16-byte aligned");
    DeviceGuard g(ctx->device);
    return model_scan_launch(ctx, d_gt, n_variants, d_counts8, (hipStream_t)stream);
}

int hpgv_assoc_model_stats_dev(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants, double *d_chisq5, double *d_p5, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0 || (n_variants > 0 && (!d_counts8 || !d_chisq5 || !d_p5))) return fail(ctx, HPGV_ERR_INVALID, "bad model stats arguments");
    if (n_variants == 0) return HPGV_OK;
    if (((uintptr_t)d_counts8 & 15) || ((uintptr_t)d_chisq5 & 7) || ((uintptr_t)d_p5 & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_counts8 must be 16-byte aligned, d_chisq5 and d_p5 8-byte aligned");
    DeviceGuard g(ctx->device);
    return model_stats_launch(ctx, d_counts8, n_variants, d_chisq5, d_p5, (hipStream_t)stream);
}

int hpgv_assoc_trend_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const int32_t *d_counts8,
                              int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_sums, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = perm_state_check(ctx)) return rc;
    if (n_variants < 0 || !d_batch_max || (n_variants > 0 && (!d_gt || !d_counts8 || !d_n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_trend_perm arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_counts8 & 15) || ((uintptr_t)d_batch_max & 7) || ((uintptr_t)d_perm_sums & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_counts8 must be 16-byte aligned, d_batch_max and d_perm_sums 8-byte aligned");
    DeviceGuard g(ctx->device);
    return perm_launch(ctx, hpgv::PERM_TREND, d_gt, n_variants, nullptr, d_counts8, nullptr, d_n_ge, d_batch_max, d_perm_sums, (hipStream_t)stream);
}

int hpgv_assoc_model(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int32_t *counts8, double *chisq5, double *p5,
                     int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_model(m_, gt, pitch, n_variants, counts8, chisq5, p5, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if ((n_ge == nullptr) != (batch_max == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "n_ge and batch_max: both (the trend permutation) or neither");
    const bool perm = batch_max != nullptr;
    if (perm) if (const int rc0 = perm_state_check(ctx)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !counts8 || !chisq5 || !p5))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_model arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0 && !perm) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    return model_finish(ctx, s, S, perm, nullptr, counts8, chisq5, p5, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_model_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                          uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *counts8, double *chisq5, double *p5,
                          int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_model_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, counts8, chisq5, p5, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if ((n_ge == nullptr) != (batch_max == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "n_ge and batch_max: both (the trend permutation) or neither");
    const bool perm = batch_max != nullptr;
    if (perm) if (const int rc0 = perm_state_check(ctx)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && (!counts8 || !chisq5 || !p5)))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_model_text arguments");
    *n_lines = 0;
    if (max_lines == 0 && !perm) return HPGV_OK;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if (max_lines > 0) {
        // the lines hpgv_assoc_text's callers drop take no part in the permutation, as in hpgv_assoc_perm_text
        rc = perm ? text_front_skip(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S)
                  : text_front(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S);
        if (rc) return rc;
    }
    return model_finish(ctx, s, S, perm, K.bytes(), counts8, chisq5, p5, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                    int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2, double *odds, double *chisq, double *p,
                    int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_perm(m_, gt, pitch, n_variants, is_x, A1, A2, U1, U2, odds, chisq, p, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = perm_state_check(ctx)) return rc0;
    if (n_variants < 0 || !batch_max || (n_variants > 0 && (!gt || !A1 || !A2 || !U1 || !U2 || !odds || !chisq || !p || !n_ge)))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_perm arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, is_x, &S))) return rc;
    return perm_finish(ctx, s, S, nullptr, A1, A2, U1, U2, odds, chisq, p, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                         uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *A1, int32_t *A2,
                         int32_t *U1, int32_t *U2, double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_perm_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, A1, A2, U1, U2, odds, chisq, p, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = perm_state_check(ctx)) return rc0;
    if (!n_lines || !batch_max || max_lines < 0 || (text_bytes > 0 && !text) ||
        (max_lines > 0 && (!A1 || !A2 || !U1 || !U2 || !odds || !chisq || !p || !n_ge)))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_perm_text arguments");
    *n_lines = 0;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if (max_lines > 0 && (rc = text_front_skip(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S))) return rc;
    return perm_finish(ctx, s, S, K.bytes(), A1, A2, U1, U2, odds, chisq, p, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

/* ---- TDT, family flips ------------------------------------------------------------------------------------------- */

int hpgv_set_tdt_flips(hpgv_ctx *ctx, const uint8_t *flips, int n_perms) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_tdt_flips(m_, flips, n_perms))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->tdt.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_families has not been called");
    if (n_perms < 0 || (n_perms > 0 && !flips)) return fail(ctx, HPGV_ERR_INVALID, "bad tdt_flips arguments");
    if (n_perms > kMaxPerms) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d permutations: at most %d per call", n_perms, kMaxPerms);
    if (n_perms == 0) { ctx->n_flips = ctx->flip_rows = ctx->flip_pitch = 0; return HPGV_OK; }
    const hpgv::TdtPlan &P = ctx->tdt_plan;
    // |t1_f - t2_f| <= 2 x children must fit the i8 operand
    if (P.max_children > 63) return fail(ctx, HPGV_ERR_UNSUPPORTED, "a family with %d counted children: at most 63 under family flips", P.max_children);
    // the family behind every K position: the fast trios in plane order, then the slow families; -1 = pad
    const size_t kpitch = (size_t)P.p16 + round_up((size_t)P.n_slow_families, 16), rows = round_up((size_t)n_perms, 16);
    std::vector<int32_t> fam_of_k(kpitch, -1);
    for (size_t t = 0; t < P.fast_family.size(); ++t) fam_of_k[t] = P.fast_family[t];
    for (size_t k = 0; k < P.slow_family.size(); ++k) fam_of_k[(size_t)P.p16 + k] = P.slow_family[k];
    const size_t nf = (size_t)ctx->tdt_families;
    std::vector<uint8_t> laid(rows * kpitch, 0);
    for (int q = 0; q < n_perms; ++q) {
        const uint8_t *src = flips + (size_t)q * nf;
        uint8_t *dst = laid.data() + (size_t)q * kpitch;
        for (size_t k = 0; k < kpitch; ++k) {
            const int32_t f = fam_of_k[k];
            if (f < 0) continue;
            if (src[f] > 1) return fail(ctx, HPGV_ERR_INVALID, "flip %u of permutation %d, family %d: flips are 0 or 1", (unsigned)src[f], q, (int)f);
            dst[k] = src[f] ? 0xFF : 0x01;               // i8: flipped -1, kept +1
        }
    }
    DeviceGuard g(ctx->device);
    ctx->n_flips = ctx->flip_rows = ctx->flip_pitch = 0;
    {
        const hipError_t e = ctx->d_flips.reserve(laid.size() + 16);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, HPGV_ERR_NOMEM, "the sign matrix (%zu bytes) does not fit the device", laid.size()); }
        HIPCHK(ctx, e);
    }
    if (!laid.empty()) HIPCHK(ctx, hipMemcpy(ctx->d_flips.p, laid.data(), laid.size(), hipMemcpyHostToDevice));
    ctx->n_flips = n_perms; ctx->flip_rows = (int)rows; ctx->flip_pitch = (int)kpitch;
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_tdt_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_tu,
                      int32_t *d_n_ge, double *d_batch_max, int32_t *d_perm_tu, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = flip_state_check(ctx)) return rc;
    if (n_variants < 0 || !d_batch_max || (n_variants > 0 && (!d_gt || !d_tu || !d_n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad tdt_perm arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_tu & 7) || ((uintptr_t)d_batch_max & 7) || ((uintptr_t)d_perm_tu & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt must be 16-byte aligned, d_tu, d_batch_max and d_perm_tu 8-byte aligned");
    DeviceGuard g(ctx->device);
    // the slow families' differences: the context's own scratch, grown after the stream that may still read it
    const size_t tail = (size_t)n_variants * (size_t)flip_tail_pitch(ctx);
    if (tail) HIPCHK(ctx, ctx->d_flip_tail.reserve_after_sync((hipStream_t)stream, tail + 16, tail + tail / 4 + 256));
    return flip_launch(ctx, d_gt, n_variants, d_is_x, d_tu, nullptr, ctx->d_flip_tail.as<int8_t>(), d_n_ge, d_batch_max, d_perm_tu, (hipStream_t)stream);
}

int hpgv_tdt_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                  int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_tdt_perm(m_, gt, pitch, n_variants, is_x, t1, t2, odds, chisq, p, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = flip_state_check(ctx)) return rc0;
    if (n_variants < 0 || !batch_max || (n_variants > 0 && (!gt || !t1 || !t2 || !odds || !chisq || !p || !n_ge)))
        return fail(ctx, HPGV_ERR_INVALID, "bad tdt_perm arguments");
    if (pitch < (size_t)ctx->tdt.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->tdt.n_samples);
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_TDT, ctx->tdt, gt, pitch, n_variants, is_x, &S))) return rc;
    return flip_finish(ctx, s, S, nullptr, t1, t2, odds, chisq, p, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_tdt_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                       uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *t1, int32_t *t2,
                       double *odds, double *chisq, double *p, int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_tdt_perm_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, t1, t2, odds, chisq, p, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = flip_state_check(ctx)) return rc0;
    if (!n_lines || !batch_max || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && (!t1 || !t2 || !odds || !chisq || !p || !n_ge)))
        return fail(ctx, HPGV_ERR_INVALID, "bad tdt_perm_text arguments");
    *n_lines = 0;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if (max_lines > 0 && (rc = text_front_skip(ctx, s, HPGV_LAYOUT_TDT, ctx->tdt, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S))) return rc;
    return flip_finish(ctx, s, S, K.bytes(), t1, t2, odds, chisq, p, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only helpers: no GPU call, usable without a device ------------------------------------------------------- */

int hpgv_perm_labels_shuffle(const uint8_t *condition, int n_samples, int n_perms, uint64_t seed, uint8_t *labels_out) {
    if (n_samples < 0 || n_perms < 0 || (n_samples > 0 && !condition) || ((size_t)n_samples * (size_t)n_perms > 0 && !labels_out)) return HPGV_ERR_INVALID;
    try {
        std::vector<int32_t> cols;
        std::vector<uint8_t> base;
        for (int j = 0; j < n_samples; ++j)
            if (condition[j] == HPGV_COND_AFFECTED || condition[j] == HPGV_COND_UNAFFECTED) { cols.push_back(j); base.push_back(condition[j] == HPGV_COND_AFFECTED ? 1 : 0); }
        const size_t nc = cols.size();
        std::vector<uint8_t> y(nc);
        for (int q = 0; q < n_perms; ++q) {
            uint8_t *row = labels_out + (size_t)q * (size_t)n_samples;
            memset(row, 0, (size_t)n_samples);
            y = base;
            // the row's stream: key = SplitMix64(seed ^ SplitMix64(q)); draw number i of the row = SplitMix64(key + i)
            const uint64_t key = splitmix64(seed ^ splitmix64((uint64_t)q));
            uint64_t draw = 0;
            for (size_t i = nc; i > 1; --i) {
                // Fisher-Yates: position i - 1 swaps with j uniform in [0, i): the high 64 bits of draw x i (bias below i / 2^64)
                const uint64_t r = splitmix64(key + draw++);
                const size_t j = (size_t)(((unsigned __int128)r * (unsigned __int128)i) >> 64);
                std::swap(y[i - 1], y[j]);
            }
            for (size_t k = 0; k < nc; ++k) row[cols[k]] = y[k];
        }
    } catch (...) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

int hpgv_perm_labels_shuffle_within(const uint8_t *condition, const int32_t *stratum_of_sample, int n_samples, int n_perms, uint64_t seed, uint8_t *labels_out) {
    if (n_samples < 0 || n_perms < 0 || (n_samples > 0 && (!condition || !stratum_of_sample)) || ((size_t)n_samples * (size_t)n_perms > 0 && !labels_out)) return HPGV_ERR_INVALID;
    try {
        // the cohort columns that are in a stratum, by (stratum, VCF column); `ends`: where each stratum's run ends
        std::vector<int32_t> cols;
        for (int j = 0; j < n_samples; ++j)
            if ((condition[j] == HPGV_COND_AFFECTED || condition[j] == HPGV_COND_UNAFFECTED) && stratum_of_sample[j] >= 0) cols.push_back(j);
        std::stable_sort(cols.begin(), cols.end(), [&](int32_t a, int32_t b) { return stratum_of_sample[a] < stratum_of_sample[b]; });
        const size_t nc = cols.size();
        std::vector<size_t> ends;
        for (size_t k = 0; k < nc; ++k)
            if (k + 1 == nc || stratum_of_sample[cols[k + 1]] != stratum_of_sample[cols[k]]) ends.push_back(k + 1);
        std::vector<uint8_t> base(nc), y(nc);
        for (size_t k = 0; k < nc; ++k) base[k] = condition[cols[k]] == HPGV_COND_AFFECTED ? 1 : 0;
        for (int q = 0; q < n_perms; ++q) {
            uint8_t *row = labels_out + (size_t)q * (size_t)n_samples;
            // outside the strata: the observed label of a cohort column, 0 for the others
            for (int j = 0; j < n_samples; ++j) row[j] = condition[j] == HPGV_COND_AFFECTED ? 1 : 0;
            y = base;
            // the row's stream is hpgv_perm_labels_shuffle's; the strata take their draws from it one after the other, in ascending order
            const uint64_t key = splitmix64(seed ^ splitmix64((uint64_t)q));
            uint64_t draw = 0;
            size_t lo = 0;
            for (const size_t hi : ends) {
                for (size_t i = hi - lo; i > 1; --i) {
                    const uint64_t r = splitmix64(key + draw++);
                    const size_t j = (size_t)(((unsigned __int128)r * (unsigned __int128)i) >> 64);
                    std::swap(y[lo + i - 1], y[lo + j]);
                }
                lo = hi;
            }
            for (size_t k = 0; k < nc; ++k) row[cols[k]] = y[k];
        }
    } catch (...) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

int hpgv_perm_order_shuffle(const uint8_t *condition, int n_samples, int n_perms, uint64_t seed, int32_t *order_out) {
    if (n_samples < 0 || n_perms < 0 || (n_samples > 0 && !condition) || ((size_t)n_samples * (size_t)n_perms > 0 && !order_out)) return HPGV_ERR_INVALID;
    try {
        std::vector<int32_t> cols;
        for (int j = 0; j < n_samples; ++j)
            if (condition[j] == HPGV_COND_AFFECTED || condition[j] == HPGV_COND_UNAFFECTED) cols.push_back(j);
        const size_t nc = cols.size();
        std::vector<int32_t> y(nc);
        for (int q = 0; q < n_perms; ++q) {
            int32_t *row = order_out + (size_t)q * (size_t)n_samples;
            for (int j = 0; j < n_samples; ++j) row[j] = j;
            y = cols;
            // the keys, the draws and the walk of hpgv_perm_labels_shuffle, over the cohort columns in place of their labels
            const uint64_t key = splitmix64(seed ^ splitmix64((uint64_t)q));
            uint64_t draw = 0;
            for (size_t i = nc; i > 1; --i) {
                const uint64_t r = splitmix64(key + draw++);
                const size_t j = (size_t)(((unsigned __int128)r * (unsigned __int128)i) >> 64);
                std::swap(y[i - 1], y[j]);
            }
            for (size_t k = 0; k < nc; ++k) row[cols[k]] = y[k];
        }
    } catch (...) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

int hpgv_perm_flips_shuffle(int n_families, int n_perms, uint64_t seed, uint8_t *flips_out) {
    if (n_families < 0 || n_perms < 0 || ((size_t)n_families * (size_t)n_perms > 0 && !flips_out)) return HPGV_ERR_INVALID;
    for (int q = 0; q < n_perms; ++q) {
        uint8_t *row = flips_out + (size_t)q * (size_t)n_families;
        // the row's stream is the label rows': key = SplitMix64(seed ^ SplitMix64(q)); word number w = SplitMix64(key + w) holds the
        // flips of families 64 w .. 64 w + 63, family f in bit f & 63
        const uint64_t key = splitmix64(seed ^ splitmix64((uint64_t)q));
        uint64_t word = 0;
        for (int f = 0; f < n_families; ++f) {
            if ((f & 63) == 0) word = splitmix64(key + (uint64_t)(f >> 6));
            row[f] = (uint8_t)((word >> (f & 63)) & 1u);
        }
    }
    return HPGV_OK;
}

int hpgv_perm_pvalues(const double *t_obs, int n_variants, const int32_t *n_ge, const double *t_max, int n_perms, double *emp1, double *emp2) {
    if (n_variants < 0 || n_perms < 1 || !t_max || (n_variants > 0 && (!t_obs || !n_ge || !emp1 || !emp2))) return HPGV_ERR_INVALID;
    try {
        std::vector<double> sorted(t_max, t_max + n_perms);
        std::sort(sorted.begin(), sorted.end());
        const double denom = (double)n_perms + 1.0;
        for (int v = 0; v < n_variants; ++v) {
            const double t = t_obs[v];
            if (t != t) { emp1[v] = emp2[v] = t; continue; }
            // permutations whose maximum is >= t: those from the first element not below t on
            const size_t ge = (size_t)(sorted.end() - std::lower_bound(sorted.begin(), sorted.end(), t));
            emp1[v] = ((double)n_ge[v] + 1.0) / denom;
            emp2[v] = ((double)ge + 1.0) / denom;
        }
    } catch (...) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

}  // extern "C"
