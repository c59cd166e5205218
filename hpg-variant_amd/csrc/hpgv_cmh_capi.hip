// hpgv_cmh_capi.hip -- C ABI of the stratified association (include/hpgv.h "stratified association"): the strata of a context, the
// device-resident launches of k_assoc_cmh_tables and k_assoc_cmh_stats, the synchronous entry points on a host batch and on a
// text -- built as hpgv_assoc_perm's are: arguments, a slot, stage_chain / text_front_skip, then cmh_finish, whose scratch
// perm_plan (hpgv_internal.h) lays out in Slot::perm with the tables as its per-row tail -- and the host-only fit.  The permutation
// within strata (k_assoc_cmh_perm) hangs on the same units: its k-step lists are built with the stratum image, its launch follows
// the two of cmh_launch in cmh_finish, and n_ge / batch_max are the front parts of the same plan.
#include "hpgv_internal.h"
#include "hpgv_assoc_cmh_kernels.h"
#include "hpgv_assoc_cmh_perm_kernels.h"

namespace {

static_assert(sizeof(hpgv_cmh_result) == 72 && offsetof(hpgv_cmh_result, chisq) == 8 && offsetof(hpgv_cmh_result, p_bd) == 64, "the record of include/hpgv.h");

int cmh_state_check(const hpgv_ctx *ctx) {
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (ctx->n_strata <= 0) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_strata has not been called (a new cohort drops the strata)");
    return HPGV_OK;
}

// the two launches on `st`: the tables in the smallest form that covers the image in one pass (NT = 8 and several passes beyond 64
// strata), then the records
int cmh_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, hpgv_cmh_result *d_out, int32_t *d_tables, hipStream_t st) {
    if (n_variants == 0) return HPGV_OK;
    hpgv::CmhArgs A;
    A.gt = d_gt; A.pitch = ctx->assoc.pitch; A.chunks = ctx->assoc.chunks; A.n_variants = n_variants; A.is_x = d_is_x;
    A.image = ctx->d_strata.as<uint8_t>(); A.image_rows = ctx->strata_rows; A.n_strata = ctx->n_strata; A.tables = (int4 *)d_tables;
    const int tiles = ctx->strata_rows / 16, nt = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 8;
    const dim3 grid((unsigned)((n_variants + hpgv::PERM_VT - 1) / hpgv::PERM_VT), (unsigned)((tiles + nt - 1) / nt));
    // (option "profile": the tables are the scan time, the records the statistics time of hpgv_last_kernel_ms)
    int rc = launch_profiled(ctx, st, 0, [&] {
        if (nt == 1) hipLaunchKernelGGL(hpgv::k_assoc_cmh_tables<1>, grid, dim3(256), 0, st, A);
        else if (nt == 2) hipLaunchKernelGGL(hpgv::k_assoc_cmh_tables<2>, grid, dim3(256), 0, st, A);
        else if (nt == 4) hipLaunchKernelGGL(hpgv::k_assoc_cmh_tables<4>, grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL(hpgv::k_assoc_cmh_tables<8>, grid, dim3(256), 0, st, A);
    });
    if (rc) return rc;
    return launch_profiled(ctx, st, 1, [&] {
        hipLaunchKernelGGL(hpgv::k_assoc_cmh_stats, dim3((unsigned)((n_variants + 255) / 256)), dim3(256), 0, st, (const int4 *)d_tables, n_variants, ctx->n_strata, d_out);
    });
}

int cmh_perm_state_check(const hpgv_ctx *ctx) {
    if (const int rc = cmh_state_check(ctx)) return rc;
    if (ctx->n_perms <= 0) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_perm_labels has not been called (a new cohort drops the labels)");
    return HPGV_OK;
}

// the permutation within strata on `st`: n_ge and batch_max zeroed on the stream, then k_assoc_cmh_perm over (variant tiles,
// permutation passes); d_tables is what cmh_launch wrote for the same rows
int cmh_perm_launch(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_tables, const uint8_t *d_skip,
                    int32_t *d_n_ge, double *d_batch_max, double *d_perm_chisq, hipStream_t st) {
    constexpr int NT = hpgv::CMH_PERM_NT, PT = NT * 16;
    const size_t tiles = ((size_t)n_variants + hpgv::PERM_VT - 1) / hpgv::PERM_VT, passes = ((size_t)ctx->n_perms + PT - 1) / PT;
    if (tiles * passes > 0x7FFFFFFFu || passes > 65535)
        return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d variants x %d permutations in one call: give the variants in several", n_variants, ctx->n_perms);
    HIPCHK(ctx, hipMemsetAsync(d_batch_max, 0, (size_t)ctx->n_perms * sizeof(double), st));
    if (n_variants == 0) return HPGV_OK;
    HIPCHK(ctx, hipMemsetAsync(d_n_ge, 0, (size_t)n_variants * sizeof(int32_t), st));
    hpgv::CmhPermArgs A;
    A.gt = d_gt; A.pitch = ctx->assoc.pitch; A.chunks = ctx->assoc.chunks; A.n_variants = n_variants; A.is_x = d_is_x;
    A.tables = (const int4 *)d_tables; A.image = ctx->d_strata.as<uint8_t>(); A.n_strata = ctx->n_strata;
    A.step_off = ctx->d_strata_steps.as<int>(); A.step_idx = A.step_off + ctx->n_strata + 1;
    A.labels = ctx->d_perm.as<uint8_t>(); A.n_perms = ctx->n_perms; A.label_rows = ctx->perm_rows;
    A.skip = d_skip; A.n_ge = d_n_ge; A.batch_max = (unsigned long long *)d_batch_max; A.perm_chisq = d_perm_chisq;
    const dim3 grid((unsigned)tiles, (unsigned)passes);
    // (option "profile": the kernel's time is the statistics time of hpgv_last_kernel_ms)
    return launch_profiled(ctx, st, 1, [&] { hipLaunchKernelGGL(hpgv::k_assoc_cmh_perm<NT>, grid, dim3(256), 0, st, A); });
}

// the back half of hpgv_assoc_cmh, hpgv_assoc_cmh_text and their _perm forms: the laid-out matrix of a staged call -> tables,
// records, with batch_max the permutation within strata -> the caller's arrays.  skip (host, may be null): the rows whose record
// and tables in the caller's arrays stay as they were, and which take no part in the permutation (n_ge 0)
int cmh_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, hpgv_cmh_result *out, int32_t *tables, int32_t *n_ge = nullptr, double *batch_max = nullptr) {
    const bool perm = batch_max != nullptr;
    if (S.n == 0 && !perm) return HPGV_OK;
    int rc;
    const size_t n = (size_t)S.n, tab = (size_t)ctx->n_strata * 16, np = perm ? (size_t)ctx->n_perms : 0;
    PermPlan P;
    if ((rc = perm_plan(ctx, s, n, np, perm ? skip : nullptr, tab, &P))) return rc;      // the tables: the plan's tail, tab bytes per row
    HIPCHK(ctx, s->dbl.reserve_slack(n * sizeof(hpgv_cmh_result) + 16));
    hpgv_cmh_result *d_out = s->dbl.as<hpgv_cmh_result>();
    int32_t *d_tables = (int32_t *)P.d_tail;
    if ((rc = cmh_launch(ctx, S.d_laid, S.n, S.d_isx, d_out, d_tables, s->stream))) return rc;
    if (perm) {
        if ((rc = cmh_perm_launch(ctx, S.d_laid, S.n, S.d_isx, d_tables, P.d_skip, P.d_n_ge, P.d_max, nullptr, s->stream))) return rc;
        if (n) HIPCHK(ctx, hipMemcpyAsync(n_ge, P.d_n_ge, n * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(batch_max, P.d_max, np * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (n == 0) { HIPCHK(ctx, hipStreamSynchronize(s->stream)); return HPGV_OK; }
    }
    if (!skip) {
        HIPCHK(ctx, hipMemcpyAsync(out, d_out, n * sizeof(hpgv_cmh_result), hipMemcpyDeviceToHost, s->stream));
        if (tables) HIPCHK(ctx, hipMemcpyAsync(tables, d_tables, n * tab, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        return HPGV_OK;
    }
    // with skipped rows: through a copy of this call's, so that what the caller holds for them is not written
    std::vector<hpgv_cmh_result> h_out(n);
    std::vector<int32_t> h_tab(tables ? n * (tab / 4) : 0);
    HIPCHK(ctx, hipMemcpyAsync(h_out.data(), d_out, n * sizeof(hpgv_cmh_result), hipMemcpyDeviceToHost, s->stream));
    if (tables) HIPCHK(ctx, hipMemcpyAsync(h_tab.data(), d_tables, n * tab, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < n; ++i) {
        if (skip[i]) continue;
        out[i] = h_out[i];
        if (tables) memcpy(tables + i * (tab / 4), h_tab.data() + i * (tab / 4), tab);
    }
    return HPGV_OK;
}

}  // namespace

extern "C" {

int hpgv_set_strata(hpgv_ctx *ctx, const int32_t *stratum_of_sample, int n_samples, int n_strata) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_strata(m_, stratum_of_sample, n_samples, n_strata))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_strata < 0 || (n_strata > 0 && !stratum_of_sample)) return fail(ctx, HPGV_ERR_INVALID, "bad strata arguments");
    if (n_strata == 0) { ctx->n_strata = ctx->strata_rows = 0; return HPGV_OK; }
    const Layout &L = ctx->assoc;
    if (n_samples != L.n_samples) return fail(ctx, HPGV_ERR_INVALID, "strata for %d samples: the cohort has %d columns", n_samples, L.n_samples);
    if (n_strata > HPGV_CMH_MAX_STRATA) return fail(ctx, HPGV_ERR_UNSUPPORTED, "%d strata: at most %d", n_strata, (int)HPGV_CMH_MAX_STRATA);
    const size_t rows = round_up((size_t)2 * (size_t)n_strata, 16), pos_unaff = (size_t)ctx->chunksA * 16;
    std::vector<uint8_t> laid(rows * L.pitch, 0);
    // beside the image, for the permutation within strata: the 64-column k-steps that hold a member of each stratum.  The positions
    // are walked in ascending order, so a stratum's steps come out ascending
    std::vector<std::vector<int32_t>> steps_of((size_t)n_strata);
    for (size_t pos = 0; pos < L.pitch; ++pos) {
        const int32_t j = L.col_of_pos[pos];
        if (j < 0) continue;
        const int32_t k = stratum_of_sample[j];
        if (k < 0) continue;
        if (k >= n_strata) return fail(ctx, HPGV_ERR_INVALID, "stratum %d of column %d: strata are 0 .. %d", (int)k, (int)j, n_strata - 1);
        laid[((size_t)2 * (size_t)k + (pos < pos_unaff ? 0 : 1)) * L.pitch + pos] = 1;      // the affected columns come first in the layout
        std::vector<int32_t> &sk = steps_of[(size_t)k];
        if (sk.empty() || sk.back() != (int32_t)(pos / 64)) sk.push_back((int32_t)(pos / 64));
    }
    std::vector<int32_t> csr((size_t)n_strata + 1, 0);
    for (int k = 0; k < n_strata; ++k) {
        csr.insert(csr.end(), steps_of[(size_t)k].begin(), steps_of[(size_t)k].end());
        csr[(size_t)k + 1] = (int32_t)(csr.size() - (size_t)n_strata - 1);      // (at most HPGV_CMH_MAX_STRATA x pitch / 64 entries)
    }
    DeviceGuard g(ctx->device);
    ctx->n_strata = ctx->strata_rows = 0;
    {
        hipError_t e = ctx->d_strata.reserve(laid.size());
        if (e == hipSuccess) e = ctx->d_strata_steps.reserve(csr.size() * sizeof(int32_t));
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(ctx, HPGV_ERR_NOMEM, "the stratum image (%zu bytes) does not fit the device", laid.size()); }
        HIPCHK(ctx, e);
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_strata.p, laid.data(), laid.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->d_strata_steps.p, csr.data(), csr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    ctx->n_strata = n_strata; ctx->strata_rows = (int)rows;
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_cmh_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, hpgv_cmh_result *d_out, int32_t *d_tables, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = cmh_state_check(ctx)) return rc;
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_out))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_cmh arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_tables & 15))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_tables must be 16-byte aligned, d_out 8-byte aligned");
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    if (!d_tables) {
        // the context's own scratch, grown after the stream that may still read it
        const size_t need = (size_t)n_variants * (size_t)ctx->n_strata * 16;
        HIPCHK(ctx, ctx->d_cmh_tables.reserve_after_sync((hipStream_t)stream, need + 16, need + need / 4 + 256));
        d_tables = ctx->d_cmh_tables.as<int32_t>();
    }
    return cmh_launch(ctx, d_gt, n_variants, d_is_x, d_out, d_tables, (hipStream_t)stream);
}

int hpgv_assoc_cmh(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x, hpgv_cmh_result *out, int32_t *tables) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_cmh(m_, gt, pitch, n_variants, is_x, out, tables))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = cmh_state_check(ctx)) return rc0;
    if (n_variants < 0 || (n_variants > 0 && (!gt || !out))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_cmh arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, is_x, &S))) return rc;
    return cmh_finish(ctx, s, S, nullptr, out, tables);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_cmh_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                        uint64_t *line_off, uint32_t *field_off, int32_t *status, hpgv_cmh_result *out, int32_t *tables) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_cmh_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, out, tables))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = cmh_state_check(ctx)) return rc0;
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !out)) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_cmh_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = text_front_skip(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S))) return rc;
    return cmh_finish(ctx, s, S, K.bytes(), out, tables);
    HPGV_ABI_CATCH(ctx)
}

/* ---- permutation within strata ------------------------------------------------------------------------------------ */

int hpgv_assoc_cmh_perm_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, const int32_t *d_tables,
                            int32_t *d_n_ge, double *d_batch_max, double *d_perm_chisq, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc = cmh_perm_state_check(ctx)) return rc;
    if (n_variants < 0 || !d_batch_max || (n_variants > 0 && (!d_gt || !d_tables || !d_n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_cmh_perm arguments");
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_tables & 15) || ((uintptr_t)d_batch_max & 7) || ((uintptr_t)d_perm_chisq & 7))
        return fail(ctx, HPGV_ERR_INVALID, "d_gt and d_tables must be 16-byte aligned, d_batch_max and d_perm_chisq 8-byte aligned");
    DeviceGuard g(ctx->device);
    return cmh_perm_launch(ctx, d_gt, n_variants, d_is_x, d_tables, nullptr, d_n_ge, d_batch_max, d_perm_chisq, (hipStream_t)stream);
}

int hpgv_assoc_cmh_perm(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                        hpgv_cmh_result *out, int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc_cmh_perm(m_, gt, pitch, n_variants, is_x, out, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = cmh_perm_state_check(ctx)) return rc0;
    if (n_variants < 0 || !batch_max || (n_variants > 0 && (!gt || !out || !n_ge))) return fail(ctx, HPGV_ERR_INVALID, "bad assoc_cmh_perm arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_chain(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, is_x, &S))) return rc;
    return cmh_finish(ctx, s, S, nullptr, out, nullptr, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_cmh_perm_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                             uint64_t *line_off, uint32_t *field_off, int32_t *status, hpgv_cmh_result *out, int32_t *n_ge, double *batch_max) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_cmh_perm_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, out, n_ge, batch_max))
    if (!ctx) return HPGV_ERR_INVALID;
    if (const int rc0 = cmh_perm_state_check(ctx)) return rc0;
    if (!n_lines || !batch_max || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && (!out || !n_ge)))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_cmh_perm_text arguments");
    *n_lines = 0;
    TextSkip K;                                  // (before the lease)
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if (max_lines > 0 && (rc = text_front_skip(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &K, &S))) return rc;
    return cmh_finish(ctx, s, S, K.bytes(), out, nullptr, n_ge, batch_max);
    HPGV_ABI_CATCH(ctx)
}

/* ---- host-only: no GPU call, usable without a device ------------------------------------------------------------- */

int hpgv_cmh_fit(const int32_t *tables, int n_strata, hpgv_cmh_result *out) {
    if (n_strata < 0 || !out || (n_strata > 0 && !tables)) return HPGV_ERR_INVALID;
    try {
        std::vector<int4> t((size_t)n_strata);                       // (the caller's integers need not be 16-byte aligned)
        for (int k = 0; k < n_strata; ++k) {
            const int32_t *q = tables + 4 * (size_t)k;
            if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0) return HPGV_ERR_INVALID;
            t[(size_t)k] = make_int4(q[0], q[1], q[2], q[3]);
        }
        *out = hpgv::cmh_fit_one(t.data(), n_strata);
    } catch (...) { return HPGV_ERR_NOMEM; }
    return HPGV_OK;
}

}  // extern "C"
