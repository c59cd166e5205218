// hpgv_tool_capi.hip -- C ABI of the tools' synchronous entry points (include/hpgv.h): association, TDT, statistics,
// Mendelian errors and the epistasis dataset on a host batch (hpgv_assoc, ...) or on a text (hpgv_assoc_text, ...).  An
// entry point checks its arguments, leases a slot, puts the matrix on the device -- a batch through stage_batch (batch_sources
// for a one-pass kernel, stage_chain for the kernel chain), a text through text_front (hpgv_text_capi.hip) -- and hands the
// result (a Staged) to its tool's back half, which is written once for both.  stage_chain and the two halves of the association
// and TDT chains are shared with the permutation and LD entry points (hpgv_perm_capi.hip, hpgv_ld_capi.hip).
#include "hpgv_internal.h"
#include "hpgv_batch_kernels.h"
#include <cstddef>
#include <utility>

namespace {

// ---- the fused per-batch path (hpgv_batch_kernels.h) ---------------------------------------------------------------
// device-visible address of host pointer p when [p, p + bytes) is page-locked (hipHostMalloc / hipHostRegister) or device
// memory; nullptr for ordinary pageable memory
static const void *mapped_view(const void *p, size_t bytes) {
    if (!p || bytes == 0) return nullptr;
    const void *ends[2] = {p, (const char *)p + bytes - 1};
    const void *dev0 = nullptr;
    for (int k = 0; k < 2; ++k) {
        hipPointerAttribute_t a;
        memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, ends[k]) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (a.type != hipMemoryTypeHost && a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) return nullptr;
        if (!a.devicePointer) return nullptr;
        if (k == 0) dev0 = a.devicePointer;
    }
    return dev0;
}

static bool batch_fused_ok(const hpgv_ctx *ctx, int n_samples) {
    return ctx->batch_fused && (size_t)n_samples + 32 <= (size_t)ctx->batch_lds_max;
}

// what a batch entry point reads of the caller's matrix (n_variants > 0): the last row need not be a whole pitch
static size_t batch_bytes(int n_variants, size_t pitch, int n_samples) { return (size_t)(n_variants - 1) * pitch + (size_t)n_samples; }

// sources of a fused call: the caller's buffers as they are when the device can read them, the slot's copies otherwise
static int batch_sources(hpgv_ctx *ctx, Slot *s, const uint8_t *gt, size_t pitch, int n_variants, int n_samples, const uint8_t *is_x,
                         Staged *S) {
    const size_t bytes = batch_bytes(n_variants, pitch, n_samples);
    // page-locked rows are read in place by the kernel -- unless batch_copy asks for the copy engine first (it moves 2 MB in
    // 35 us where the kernel's own reads over the bus take 44; the kernel then runs on device memory)
    const void *src = ctx->batch_copy ? nullptr : mapped_view(gt, bytes);
    if (!src) {
        HIPCHK(ctx, s->raw.reserve_slack(bytes + 16));
        HIPCHK(ctx, hipMemcpyAsync(s->raw.p, gt, bytes, hipMemcpyHostToDevice, s->stream));
        src = s->raw.p;
    }
    const void *x = nullptr;
    if (is_x) {
        x = mapped_view(is_x, (size_t)n_variants);
        if (!x) {
            HIPCHK(ctx, s->isx.reserve_slack((size_t)n_variants));
            HIPCHK(ctx, hipMemcpyAsync(s->isx.p, is_x, (size_t)n_variants, hipMemcpyHostToDevice, s->stream));
            x = s->isx.p;
        }
    }
    S->d_raw = (const uint8_t *)src; S->raw_pitch = pitch; S->d_isx = (const uint8_t *)x;
    S->n = n_variants; S->out_stride = (size_t)n_variants;
    return HPGV_OK;
}

// a batch on the device.  one_pass: for a kernel that reads the raw rows itself (batch_sources); else for the kernel chain
// (stage_chain, below the back halves)
static int stage_batch(hpgv_ctx *ctx, Slot *s, bool one_pass, int which, const Layout &L, const uint8_t *gt, size_t pitch,
                       int n_variants, const uint8_t *is_x, Staged *S) {
    if (one_pass) return batch_sources(ctx, s, gt, pitch, n_variants, L.n_samples, is_x, S);
    return stage_chain(ctx, s, which, L, gt, pitch, n_variants, is_x, S);
}

// ---- k_stats_all on a matrix the device can read (the tokenizer's raw matrix, or a host batch through batch_sources): every
// output is optional except the per-variant counters' record block, which the kernel always produces -------------------
struct StatsAllOut {
    int32_t *counts8 = nullptr; double *hwe_chi2 = nullptr, *hwe_p = nullptr;        // [n]
    int32_t *sample_missing = nullptr;                                                // [n_samples], accumulated into
    int32_t *mendel_errors = nullptr;                                                 // [n]
    int32_t *child_errors = nullptr;                                                  // [n_trios], accumulated into
    int32_t *group_counts8 = nullptr; double *group_hwe_chi2 = nullptr, *group_hwe_p = nullptr;   // [g * out_stride + v]
};
// LDS the kernel needs for this cohort; 0 when it cannot run (row window + column counters + trio counters too large)
static size_t stats_all_lds(const hpgv_ctx *ctx, bool mendel) {
    const size_t ns = (size_t)ctx->stats.n_samples;
    const size_t need = (ns + 32 + 15) / 16 * 16 + (ns + 15) / 16 * 16 + (mendel ? (size_t)ctx->mendel_pchunks * 16 : 0) + 16;
    return (ctx->batch_fused && need <= (size_t)ctx->batch_lds_max) ? need : 0;
}
static int stats_all_call(hpgv_ctx *ctx, Slot *s, const Staged &S, const StatsAllOut &O) {
    const int n_variants = S.n;
    const size_t n = (size_t)n_variants, group_stride = S.out_stride;
    const int ns = ctx->stats.n_samples;
    const bool want_mendel = O.mendel_errors || O.child_errors;
    const size_t ng = O.group_counts8 ? ctx->sg_off.size() : 0, nt = want_mendel ? (size_t)ctx->mendel_trios : 0;
    const size_t rec_bytes = (1 + ng) * n * sizeof(hpgv::BatchStatsRec);
    HIPCHK(ctx, s->res.reserve(rec_bytes + n * sizeof(int32_t) + 64));
    const bool want_sm = O.sample_missing && ns > 0, want_ce = O.child_errors && nt > 0;
    HIPCHK(ctx, s->smiss.reserve_slack(((size_t)ns + nt + 16) * sizeof(int32_t)));
    int32_t *d_sm = s->smiss.as<int32_t>(), *d_ce = d_sm + ns;
    if (want_sm || want_ce) HIPCHK(ctx, hipMemsetAsync(d_sm, 0, ((size_t)ns + nt) * sizeof(int32_t), s->stream));
    hpgv::StatsAllArgs A;
    memset(&A, 0, sizeof A);
    A.src = S.d_raw; A.src_pitch = S.raw_pitch; A.n_variants = n_variants; A.n_samples = ns;
    A.is_x = S.d_isx;
    A.out = (hpgv::BatchStatsRec *)s->res.d;
    A.sample_missing = want_sm ? d_sm : nullptr;
    if (want_mendel) {
        A.mendel_cols = ctx->mendel.d_col_of_pos(); A.pchunks = ctx->mendel_pchunks; A.n_trios = ctx->mendel_trios;
        A.luts = ctx->mendel_luts; A.male_plane = ctx->d_mendel_male;
        A.mendel_errors = O.mendel_errors ? (int32_t *)((char *)s->res.d + rec_bytes) : nullptr;
        A.child_errors = want_ce ? d_ce : nullptr;
    }
    if (ng) {
        A.group_cols = ctx->sgroups.d_col_of_pos(); A.n_groups = (int)ng;
        A.group_chunk0 = ctx->d_sg_chunks.as<int32_t>(); A.group_chunks = A.group_chunk0 + ng;
        A.group_out = (hpgv::BatchStatsRec *)s->res.d + n;
    }
    // a band of rows per workgroup keeps the column counters in LDS across rows; short batches stay one row per workgroup
    // (one band per workgroup slot of the chip, about three per compute unit: the band's end -- its column counters' atomics --
    // costs as much as several rows, and fewer workgroups than slots leave units idle: 16 000 rows, 8 / 21 / 42 per band:
    // 105 / 65 / 84 us)
    int rows = (n_variants + 3 * ctx->n_cus - 1) / (3 * ctx->n_cus);
#ifdef HPGV_ABLATION
    if (ctx->stats_rows) rows = (int)ctx->stats_rows;               // tuning: the band length
#endif
    rows = rows < 1 ? 1 : (rows > 255 ? 255 : rows);
    A.rows_per_block = rows; A.lds_row = (int)(((size_t)ns + 32 + 15) / 16 * 16);
    // columns owned by threads across the band (hpgv_statsall_kernels.h); what that kernel does not take -- unaligned rows,
    // very wide cohorts, many groups -- goes to the row-staging kernel
    if (!ctx->stats_all2 || hpgv_launch_stats_all2(ctx, A, s->row_cnt, s->stream) != 0) {
        const size_t lds = stats_all_lds(ctx, want_mendel);
        hipLaunchKernelGGL(hpgv::k_stats_all, dim3((unsigned)((n_variants + rows - 1) / rows)), dim3(256), lds, s->stream, A);
    }
    HIPCHK(ctx, hipGetLastError());
    std::vector<int32_t> acc;
    if (want_sm || want_ce) {
        acc.resize((size_t)ns + nt);
        HIPCHK(ctx, hipMemcpyAsync(acc.data(), d_sm, acc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    const hpgv::BatchStatsRec *r = (const hpgv::BatchStatsRec *)s->res.h;
    if (O.counts8)
        for (size_t i = 0; i < n; ++i) {
            memcpy(O.counts8 + 8 * i, r[i].c8, 8 * sizeof(int32_t));
            if (O.hwe_chi2) { O.hwe_chi2[i] = r[i].hwe_chi2; O.hwe_p[i] = r[i].hwe_p; }
        }
    for (size_t k = 0; k < ng; ++k)
        for (size_t i = 0; i < n; ++i) {
            const hpgv::BatchStatsRec &q = r[n + k * n + i];
            memcpy(O.group_counts8 + (k * group_stride + i) * 8, q.c8, 8 * sizeof(int32_t));
            if (O.group_hwe_chi2) { O.group_hwe_chi2[k * group_stride + i] = q.hwe_chi2; O.group_hwe_p[k * group_stride + i] = q.hwe_p; }
        }
    if (O.mendel_errors) memcpy(O.mendel_errors, (const char *)s->res.h + rec_bytes, n * sizeof(int32_t));
    if (want_sm) for (int j = 0; j < ns; ++j) O.sample_missing[j] += acc[(size_t)j];
    if (want_ce) for (size_t t = 0; t < nt; ++t) O.child_errors[t] += acc[(size_t)ns + t];
    return HPGV_OK;
}

// the fused kernel of one tool over a staged matrix: raw rows (read in place from page-locked memory, or the tokenizer's)
// -> layout in registers -> counts -> statistics -> packed records of rec_bytes each.  The caller has filled the tool's
// fields of A (and n_samples); when this returns the records lie in the slot's page-locked block, s->res.h
template <int KIND>
static int launch_batch(hpgv_ctx *ctx, Slot *s, const Staged &S, hpgv::BatchArgs &A, size_t rec_bytes) {
    HIPCHK(ctx, s->res.reserve((size_t)S.n * rec_bytes));
    A.src = S.d_raw; A.src_pitch = S.raw_pitch; A.n_variants = S.n; A.is_x = S.d_isx;
    A.out = s->res.d;
    const size_t lds = ((size_t)A.n_samples + 15 + 15) / 16 * 16 + 16;
    hipLaunchKernelGGL((hpgv::k_batch<KIND>), dim3((unsigned)A.n_variants), dim3(256), lds, s->stream, A);
    if (const int rc = [&] { HIPCHK(ctx, hipGetLastError()); return (int)HPGV_OK; }()) { (void)hipStreamSynchronize(s->stream); return rc; }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

// ---- the tools' back halves: from a staged matrix to the caller's arrays, written once for a batch and a text -------------

static int assoc_statistics(hpgv_ctx *ctx, int task, const int32_t *d_counts, int nv, double *d_odds, double *d_chisq, double *d_p, hipStream_t st) {
    return task == HPGV_TASK_CHISQ ? hpgv_assoc_chisq_dev(ctx, d_counts, nv, d_odds, d_chisq, d_p, st)
                                   : hpgv_assoc_fisher_dev(ctx, d_counts, nv, d_odds, d_p, st);
}

// chi-square or Fisher per variant.  A text that skipped the layout is counted by k_assoc_rows where that kernel takes
// the cohort; any matrix that skipped it goes through the fused kernel; a laid-out one through the scans' kernel chain.
// p_at (may be null): where the p-values lie on the device when this returns, p_i at p_at->first + i * p_at->second bytes
static int assoc_finish(hpgv_ctx *ctx, Slot *s, int task, const Staged &S, int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                        double *odds, double *chisq, double *p, std::pair<const char *, size_t> *p_at = nullptr) {
    int rc;
    const int nv = S.n;
    const size_t n = (size_t)nv;
    const bool chi = task == HPGV_TASK_CHISQ, rows = !S.d_laid && S.text && ctx->assoc_rows;
    if (S.d_laid) {
        ChainOut C;
        if ((rc = assoc_chain(ctx, s, task, S, &C))) return rc;
        if (p_at) *p_at = {(const char *)C.d_p, sizeof(double)};
        if ((rc = assoc_copy_out(ctx, s, task, S, C, A1, A2, U1, U2, odds, chisq, p))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        return HPGV_OK;
    }
    if (rows) {
        // the raw matrix read once by threads that own columns (k_assoc_rows), then the scans' own statistics kernels
        HIPCHK(ctx, s->tally.reserve_slack(n * 16));
        HIPCHK(ctx, s->dbl.reserve_slack(n * 3 * sizeof(double)));
        HIPCHK(ctx, s->res.reserve(n * 40 + 64));
        int32_t *d_counts = s->tally.as<int32_t>();
        double *d_odds = s->dbl.as<double>(), *d_chisq = d_odds + n, *d_p = d_odds + 2 * n;
        if (hpgv_launch_assoc_rows(ctx, S.d_raw, S.raw_pitch, nv, S.d_isx, d_counts, s->stream) == 0) {
            HIPCHK(ctx, hipGetLastError());
            if (p_at) *p_at = {(const char *)d_p, sizeof(double)};
            if ((rc = assoc_statistics(ctx, task, d_counts, nv, d_odds, d_chisq, d_p, s->stream))) { (void)hipStreamSynchronize(s->stream); return rc; }
            // results come back through the slot's page-locked block (one copy each at the bus rate), then into the caller's arrays
            char *h = (char *)s->res.h;
            HIPCHK(ctx, hipMemcpyAsync(h, d_counts, n * 16, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(ctx, hipMemcpyAsync(h + n * 16, d_odds, n * 24, hipMemcpyDeviceToHost, s->stream));
            HIPCHK(ctx, hipStreamSynchronize(s->stream));
            const int32_t *c4 = (const int32_t *)h;
            const double *dd = (const double *)(h + n * 16);
            for (size_t i = 0; i < n; ++i) { A1[i] = c4[4 * i]; A2[i] = c4[4 * i + 1]; U1[i] = c4[4 * i + 2]; U2[i] = c4[4 * i + 3]; }
            memcpy(odds, dd, n * 8);
            if (chi) memcpy(chisq, dd + n, n * 8);
            memcpy(p, dd + 2 * n, n * 8);
            return HPGV_OK;
        }
    }
    // one kernel; the only other work of the call is unpacking its records
    hpgv::BatchArgs A;
    memset(&A, 0, sizeof A);
    A.n_samples = ctx->assoc.n_samples;
    A.col_of_pos = ctx->assoc.d_col_of_pos(); A.chunks = ctx->assoc.chunks; A.chunksA = ctx->chunksA;
    A.lf = ctx->d_lf; A.rel_cut = pow(10.0, -(double)ctx->fisher_cut_exp);
    rc = chi ? launch_batch<hpgv::BATCH_CHISQ>(ctx, s, S, A, sizeof(hpgv::BatchAssocRec))
             : launch_batch<hpgv::BATCH_FISHER>(ctx, s, S, A, sizeof(hpgv::BatchAssocRec));
    if (rc) return rc;
    if (p_at) *p_at = {(const char *)s->res.d + offsetof(hpgv::BatchAssocRec, p), sizeof(hpgv::BatchAssocRec)};
    const hpgv::BatchAssocRec *r = (const hpgv::BatchAssocRec *)s->res.h;
    for (size_t i = 0; i < n; ++i) {
        A1[i] = r[i].A1; A2[i] = r[i].A2; U1[i] = r[i].U1; U2[i] = r[i].U2;
        odds[i] = r[i].odds; p[i] = r[i].p;
    }
    if (chi) for (size_t i = 0; i < n; ++i) chisq[i] = r[i].chisq;
    return HPGV_OK;
}

static int tdt_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p) {
    int rc;
    const size_t n = (size_t)S.n;
    if (!S.d_laid) {
        hpgv::BatchArgs A;
        memset(&A, 0, sizeof A);
        const hpgv::TdtPlan &P = ctx->tdt_plan;
        A.n_samples = ctx->tdt.n_samples;
        A.col_of_pos = ctx->tdt.d_col_of_pos(); A.chunks = ctx->tdt.chunks;
        A.pchunks = P.pchunks; A.p16 = P.p16; A.n_slow = P.n_slow_families; A.slow_base = P.slow_base; A.luts = P.luts;
        A.male_plane = P.d_male_plane; A.slow_off = P.d_slow_off; A.slow_male = P.d_slow_male;
        if ((rc = launch_batch<hpgv::BATCH_TDT>(ctx, s, S, A, sizeof(hpgv::BatchTdtRec)))) return rc;
        const hpgv::BatchTdtRec *r = (const hpgv::BatchTdtRec *)s->res.h;
        for (size_t i = 0; i < n; ++i) { t1[i] = r[i].t1; t2[i] = r[i].t2; odds[i] = r[i].odds; chisq[i] = r[i].chisq; p[i] = r[i].p; }
        return HPGV_OK;
    }
    ChainOut C;
    std::vector<int32_t> tu;
    if ((rc = tdt_chain(ctx, s, S, &C))) return rc;
    if ((rc = tdt_copy_out(ctx, s, S, C, &tu, odds, chisq, p))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    tdt_split_counts(tu, t1, t2);
    return HPGV_OK;
}

// the staged rows in layout `which`: as they are when they were laid out for it, else laid out anew from the raw matrix into
// the slot's `laid` -- which may move: S follows it.  The launches queued on the rows as they were run first, on the same stream
static int laid_as(hpgv_ctx *ctx, Slot *s, Staged *S, int which, const Layout &L) {
    if (S->which == which) return HPGV_OK;
    HIPCHK(ctx, s->laid.reserve_slack((size_t)S->n * L.pitch + 16));
    S->d_laid = s->laid.as<uint8_t>(); S->which = which;
    return hpgv_layout_dev(ctx, which, S->d_raw, S->raw_pitch, S->n, s->laid.as<uint8_t>(), s->stream);
}

// the statistics of a laid-out matrix by the scans' kernels, each output of O that is asked for: counters and
// Hardy-Weinberg with the per-sample missing counts, then Mendelian errors, then the counters of every phenotype group
static int stats_chain(hpgv_ctx *ctx, Slot *s, Staged S, const StatsAllOut &O) {
    int rc;
    const int nv = S.n, ns = ctx->stats.n_samples;
    const size_t n = (size_t)nv;
    std::vector<int32_t> sm, ce;
    if (O.counts8) {
        HIPCHK(ctx, s->tally.reserve_slack(n * 32));
        HIPCHK(ctx, s->dbl.reserve_slack(n * 2 * sizeof(double) + 64));
        int32_t *d_c8 = s->tally.as<int32_t>();
        double *d_chi2 = s->dbl.as<double>(), *d_p = d_chi2 + n;
        if ((rc = hpgv_stats_scan_dev(ctx, S.d_laid, nv, d_c8, s->stream))) return rc;
        if ((rc = hpgv_stats_hwe_dev(ctx, d_c8, nv, d_chi2, d_p, s->stream))) return rc;
        if (O.sample_missing && ns > 0) {
            HIPCHK(ctx, s->smiss.reserve_slack((size_t)ns * sizeof(int32_t)));
            int32_t *d_sm = s->smiss.as<int32_t>();
            HIPCHK(ctx, hipMemsetAsync(d_sm, 0, (size_t)ns * sizeof(int32_t), s->stream));
            if ((rc = hpgv_sample_missing_dev(ctx, S.d_laid, nv, d_sm, s->stream))) return rc;
            sm.resize((size_t)ns);
            HIPCHK(ctx, hipMemcpyAsync(sm.data(), d_sm, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        }
        HIPCHK(ctx, hipMemcpyAsync(O.counts8, d_c8, n * 32, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(O.hwe_chi2, d_chi2, n * 8, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipMemcpyAsync(O.hwe_p, d_p, n * 8, hipMemcpyDeviceToHost, s->stream));
    }
    if (O.mendel_errors || O.child_errors) {
        const size_t nt = (size_t)ctx->mendel_trios;
        if ((rc = laid_as(ctx, s, &S, HPGV_LAYOUT_MENDEL, ctx->mendel))) return rc;
        const uint8_t *d_gt = S.d_laid;
        HIPCHK(ctx, s->merr.reserve_slack((n + nt) * sizeof(int32_t) + 64));
        int32_t *d_err = s->merr.as<int32_t>(), *d_child = d_err + n;
        if (O.mendel_errors) {
            if ((rc = hpgv_mendel_scan_dev(ctx, d_gt, nv, S.d_isx, d_err, s->stream))) return rc;
            HIPCHK(ctx, hipMemcpyAsync(O.mendel_errors, d_err, n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        }
        if (O.child_errors && nt) {
            HIPCHK(ctx, hipMemsetAsync(d_child, 0, nt * sizeof(int32_t), s->stream));
            if ((rc = hpgv_mendel_children_dev(ctx, d_gt, nv, S.d_isx, d_child, s->stream))) return rc;
            ce.resize(nt);
            HIPCHK(ctx, hipMemcpyAsync(ce.data(), d_child, nt * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        }
    }
    if (O.group_counts8) {
        const size_t ng = ctx->sg_off.size();
        if ((rc = laid_as(ctx, s, &S, HPGV_LAYOUT_STATS_GROUPS, ctx->sgroups))) return rc;
        const uint8_t *d_gt = S.d_laid;
        HIPCHK(ctx, s->gtally.reserve_slack(ng * n * 32 + 64));
        HIPCHK(ctx, s->gdbl.reserve_slack(ng * n * 2 * sizeof(double) + 64));
        int32_t *d_g8 = s->gtally.as<int32_t>();
        double *d_ghw = s->gdbl.as<double>();
        for (size_t k = 0; k < ng; ++k) {
            if ((rc = hpgv_stats_scan_group_dev(ctx, d_gt, nv, (int)k, d_g8 + k * n * 8, s->stream))) return rc;
            if (O.group_hwe_chi2 && (rc = hpgv_stats_hwe_dev(ctx, d_g8 + k * n * 8, nv, d_ghw + k * n, d_ghw + (ng + k) * n, s->stream))) return rc;
        }
        for (size_t k = 0; k < ng; ++k) {                            // the outputs' groups lie out_stride variants apart
            HIPCHK(ctx, hipMemcpyAsync(O.group_counts8 + k * S.out_stride * 8, d_g8 + k * n * 8, n * 32, hipMemcpyDeviceToHost, s->stream));
            if (O.group_hwe_chi2) {
                HIPCHK(ctx, hipMemcpyAsync(O.group_hwe_chi2 + k * S.out_stride, d_ghw + k * n, n * 8, hipMemcpyDeviceToHost, s->stream));
                HIPCHK(ctx, hipMemcpyAsync(O.group_hwe_p + k * S.out_stride, d_ghw + (ng + k) * n, n * 8, hipMemcpyDeviceToHost, s->stream));
            }
        }
    }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    for (size_t j = 0; j < sm.size(); ++j) O.sample_missing[j] += sm[j];
    for (size_t t = 0; t < ce.size(); ++t) O.child_errors[t] += ce[t];
    return HPGV_OK;
}

// the 256-bin genotype tables of the variants whose biallelic cells do not cover every called genotype (at most `cap` of
// them; *n_multi says how many there are)
static int multi_tables(hpgv_ctx *ctx, Slot *s, const Staged &S, const int32_t *counts8, int ns, int cap, int32_t *multi_idx,
                        int32_t *multi_table, int *n_multi) {
    std::vector<int32_t> idx;
    for (int i = 0; i < S.n; ++i) {
        const int32_t *c = counts8 + 8 * (size_t)i;
        if (ns - c[4] - (c[0] + c[1] + c[2] + c[3]) > 0) idx.push_back(i);
    }
    *n_multi = (int)idx.size();
    const int m = (int)idx.size() < cap ? (int)idx.size() : cap;
    if (m <= 0) return HPGV_OK;
    const int rc = [&] {
        HIPCHK(ctx, s->multi.reserve_slack((size_t)m * 257 * sizeof(int32_t)));
        int32_t *d_idx = s->multi.as<int32_t>(), *d_tab = d_idx + m;
        HIPCHK(ctx, hipMemcpyAsync(d_idx, idx.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
        if (const int e = hpgv_genotype_table_dev(ctx, S.d_raw, S.raw_pitch, ns, d_idx, m, d_tab, s->stream)) return e;
        HIPCHK(ctx, hipMemcpyAsync(multi_table, d_tab, (size_t)m * 256 * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        return (int)HPGV_OK;
    }();
    if (rc) { (void)hipStreamSynchronize(s->stream); return rc; }    // idx is read by a queued copy
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    memcpy(multi_idx, idx.data(), (size_t)m * sizeof(int32_t));
    return HPGV_OK;
}

// every statistic O asks for, then the multi-allelic tables (n_multi non-null; they need O.counts8).  batch_stats: counters
// and Hardy-Weinberg alone from the fused per-batch kernel (get_variants_stats' shape); else a matrix that skipped the
// layout goes through ONE pass of k_stats_all (get_sample_stats' shape, stats_runner.c:197-198: the genotype bytes are read
// once), a laid-out one through the kernel chain
static int stats_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, bool batch_stats, const StatsAllOut &O, int cap,
                        int32_t *multi_idx, int32_t *multi_table, int *n_multi) {
    int rc;
    const int ns = ctx->stats.n_samples;
    if (batch_stats) {
        hpgv::BatchArgs A;
        memset(&A, 0, sizeof A);
        A.n_samples = ns;
        A.col_of_pos = ctx->stats.d_col_of_pos(); A.chunks = ctx->stats.chunks;
        if ((rc = launch_batch<hpgv::BATCH_STATS>(ctx, s, S, A, sizeof(hpgv::BatchStatsRec)))) return rc;
        const hpgv::BatchStatsRec *r = (const hpgv::BatchStatsRec *)s->res.h;
        for (size_t i = 0; i < (size_t)S.n; ++i) {
            memcpy(O.counts8 + 8 * i, r[i].c8, 8 * sizeof(int32_t));
            O.hwe_chi2[i] = r[i].hwe_chi2; O.hwe_p[i] = r[i].hwe_p;
        }
    } else if ((rc = S.d_laid ? stats_chain(ctx, s, S, O) : stats_all_call(ctx, s, S, O))) return rc;
    return n_multi ? multi_tables(ctx, s, S, O.counts8, ns, cap, multi_idx, multi_table, n_multi) : HPGV_OK;
}

// the vcf2epi rows of a matrix in the epistasis layout: cases, then controls, the 16-byte pads dropped, straight into the
// caller's rows
static int epi_rows_out(hpgv_ctx *ctx, Slot *s, const Staged &S, uint8_t *out) {
    const size_t nA = (size_t)ctx->nA, nU = (size_t)ctx->nU, width = nA + nU;
    if (S.n > 0 && width > 0) {
        const size_t segA = (size_t)ctx->chunksA * 16, dp = ctx->assoc.pitch;
        if (nA) HIPCHK(ctx, hipMemcpy2DAsync(out, width, S.d_laid, dp, nA, (size_t)S.n, hipMemcpyDeviceToHost, s->stream));
        if (nU) HIPCHK(ctx, hipMemcpy2DAsync(out + nA, width, S.d_laid + segA, dp, nU, (size_t)S.n, hipMemcpyDeviceToHost, s->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

}  // namespace

// ---- shared with hpgv_perm_capi.hip and hpgv_ld_capi.hip (hpgv_internal.h) ----------------------------------------------------

int stage_chain(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                Staged *S) {
    S->n = n_variants; S->out_stride = (size_t)n_variants;
    if (n_variants == 0) return HPGV_OK;
    // what the chain reads of the raw rows (k_layout, k_genotype_table) is the first n_samples bytes of each, byte by byte; 16 bytes
    // of room behind the last row are reserved all the same
    const size_t bytes = batch_bytes(n_variants, pitch, L.n_samples);
    HIPCHK(ctx, s->raw.reserve_slack(bytes + 16));
    HIPCHK(ctx, s->laid.reserve_slack((size_t)n_variants * L.pitch + 16));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(s->raw.p, gt, bytes, hipMemcpyHostToDevice, s->stream));
    if (is_x) {
        HIPCHK(ctx, s->isx.reserve_slack((size_t)n_variants));
        HIPCHK(ctx, hipMemcpyAsync(s->isx.p, is_x, (size_t)n_variants, hipMemcpyHostToDevice, s->stream));
        S->d_isx = s->isx.as<uint8_t>();
    }
    S->d_raw = s->raw.as<uint8_t>(); S->raw_pitch = pitch; S->d_laid = s->laid.as<uint8_t>(); S->which = which;
    return hpgv_layout_dev(ctx, which, S->d_raw, pitch, n_variants, s->laid.as<uint8_t>(), s->stream);
}

int assoc_chain(hpgv_ctx *ctx, Slot *s, int task, const Staged &S, ChainOut *C) {
    const size_t n = (size_t)S.n;
    HIPCHK(ctx, s->tally.reserve_slack(n * 16 + 16));
    HIPCHK(ctx, s->dbl.reserve_slack(n * 3 * sizeof(double) + 16));
    HIPCHK(ctx, s->ints.reserve_slack(n * 4 * sizeof(int32_t) + 16));
    C->d_tally = s->tally.as<int32_t>();
    C->d_odds = s->dbl.as<double>(); C->d_chisq = C->d_odds + n; C->d_p = C->d_odds + 2 * n;
    if (S.n == 0) return HPGV_OK;
    if (const int rc = hpgv_assoc_scan_dev(ctx, S.d_laid, S.n, S.d_isx, C->d_tally, s->stream)) return rc;
    return assoc_statistics(ctx, task, C->d_tally, S.n, C->d_odds, C->d_chisq, C->d_p, s->stream);
}

int assoc_copy_out(hpgv_ctx *ctx, Slot *s, int task, const Staged &S, const ChainOut &C, int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                   double *odds, double *chisq, double *p) {
    if (S.n == 0) return HPGV_OK;
    const size_t n = (size_t)S.n;
    int32_t *d_soa = s->ints.as<int32_t>();
    hipLaunchKernelGGL(hpgv::k_counts_to_soa, dim3((S.n + 255) / 256), dim3(256), 0, s->stream,
                       (const int4 *)C.d_tally, S.n, d_soa, d_soa + n, d_soa + 2 * n, d_soa + 3 * n);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(A1, d_soa, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(A2, d_soa + n, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(U1, d_soa + 2 * n, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(U2, d_soa + 3 * n, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(odds, C.d_odds, n * 8, hipMemcpyDeviceToHost, s->stream));
    if (task == HPGV_TASK_CHISQ) HIPCHK(ctx, hipMemcpyAsync(chisq, C.d_chisq, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(p, C.d_p, n * 8, hipMemcpyDeviceToHost, s->stream));
    return HPGV_OK;
}

int tdt_chain(hpgv_ctx *ctx, Slot *s, const Staged &S, ChainOut *C) {
    const size_t n = (size_t)S.n;
    HIPCHK(ctx, s->tally.reserve_slack(n * 8 + 16));
    HIPCHK(ctx, s->dbl.reserve_slack(n * 3 * sizeof(double) + 16));
    C->d_tally = s->tally.as<int32_t>();
    C->d_odds = s->dbl.as<double>(); C->d_chisq = C->d_odds + n; C->d_p = C->d_odds + 2 * n;
    if (S.n == 0) return HPGV_OK;
    if (const int rc = hpgv_tdt_scan_dev(ctx, S.d_laid, S.n, S.d_isx, C->d_tally, s->stream)) return rc;
    return hpgv_tdt_stats_dev(ctx, C->d_tally, S.n, C->d_odds, C->d_chisq, C->d_p, s->stream);
}

int tdt_copy_out(hpgv_ctx *ctx, Slot *s, const Staged &S, const ChainOut &C, std::vector<int32_t> *tu, double *odds, double *chisq, double *p) {
    const size_t n = (size_t)S.n;
    tu->resize(2 * n);
    if (S.n == 0) return HPGV_OK;
    HIPCHK(ctx, hipMemcpyAsync(tu->data(), C.d_tally, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(odds, C.d_odds, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(chisq, C.d_chisq, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(p, C.d_p, n * 8, hipMemcpyDeviceToHost, s->stream));
    return HPGV_OK;
}

void tdt_split_counts(const std::vector<int32_t> &tu, int32_t *t1, int32_t *t2) {
    for (size_t i = 0; 2 * i < tu.size(); ++i) { t1[i] = tu[2 * i]; t2[i] = tu[2 * i + 1]; }
}

// the fused per-batch kernels stage one raw row in LDS: ask for the whole 160 KiB where the device has it
long hpgv_batch_lds_optin(const hipDeviceProp_t &prop, long fallback) {
    const int want = 160 * 1024 - 1024;
    bool ok = true;
    ok = ok && hipFuncSetAttribute((const void *)hpgv::k_batch<hpgv::BATCH_CHISQ>, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)hpgv::k_batch<hpgv::BATCH_FISHER>, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)hpgv::k_batch<hpgv::BATCH_TDT>, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)hpgv::k_batch<hpgv::BATCH_STATS>, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)hpgv::k_stats_all, hipFuncAttributeMaxDynamicSharedMemorySize, want) == hipSuccess;
    ok = ok && (prop.sharedMemPerBlockOptin >= (size_t)want || prop.maxSharedMemoryPerMultiProcessor >= (size_t)want);
    (void)hipGetLastError();
    return ok ? want : fallback;
}

extern "C" {

/* ---- synchronous per-batch and per-text entry points: checks, slot, stage, the tool's back half --------------------- */

int hpgv_assoc(hpgv_ctx *ctx, int task, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
               int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2, double *odds, double *chisq, double *p) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_assoc(m_, task, gt, pitch, n_variants, is_x, A1, A2, U1, U2, odds, chisq, p))
    if (!ctx) return HPGV_ERR_INVALID;
    if (task != HPGV_TASK_CHISQ && task != HPGV_TASK_FISHER) return fail(ctx, HPGV_ERR_INVALID, "task must be CHISQ or FISHER");
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!gt || !A1 || !A2 || !U1 || !U2 || !odds || !p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc arguments");
    if (task == HPGV_TASK_CHISQ && n_variants > 0 && !chisq) return fail(ctx, HPGV_ERR_INVALID, "chisq output is NULL");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    const bool fused = batch_fused_ok(ctx, ctx->assoc.n_samples);
    if (fused && task == HPGV_TASK_FISHER && (rc = logfact_check(ctx))) return rc;
    Staged S;
    if ((rc = stage_batch(ctx, s, fused, HPGV_LAYOUT_ASSOC, ctx->assoc, gt, pitch, n_variants, is_x, &S))) return rc;
    return assoc_finish(ctx, s, task, S, A1, A2, U1, U2, odds, chisq, p);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_text(hpgv_ctx *ctx, int task, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                    uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *A1, int32_t *A2,
                    int32_t *U1, int32_t *U2, double *odds, double *chisq, double *p) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_text(m_, task, text, text_bytes, max_lines, n_lines, line_off, field_off, status, A1, A2, U1, U2, odds, chisq, p))
    if (!ctx) return HPGV_ERR_INVALID;
    if (task != HPGV_TASK_CHISQ && task != HPGV_TASK_FISHER) return fail(ctx, HPGV_ERR_INVALID, "task must be CHISQ or FISHER");
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) ||
        (max_lines > 0 && (!A1 || !A2 || !U1 || !U2 || !odds || !p || (task == HPGV_TASK_CHISQ && !chisq))))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    const bool fused = batch_fused_ok(ctx, ctx->assoc.n_samples);
    if (fused && task == HPGV_TASK_FISHER && (rc = logfact_check(ctx))) return rc;
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S, !fused))) return rc;
    if (S.n == 0) { HIPCHK(ctx, hipStreamSynchronize(s->stream)); return HPGV_OK; }
    return assoc_finish(ctx, s, task, S, A1, A2, U1, U2, odds, chisq, p);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_select_text(hpgv_ctx *ctx, int task, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                           uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *A1, int32_t *A2,
                           int32_t *U1, int32_t *U2, double *odds, double *chisq, double *p,
                           double p_max, int32_t *sel, uint8_t *rows_out, size_t rows_pitch, int rows_cap, int *n_sel) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_assoc_select_text(m_, task, text, text_bytes, max_lines, n_lines, line_off, field_off, status, A1, A2, U1, U2, odds,
                                                      chisq, p, p_max, sel, rows_out, rows_pitch, rows_cap, n_sel))
    if (!ctx) return HPGV_ERR_INVALID;
    if (task != HPGV_TASK_CHISQ && task != HPGV_TASK_FISHER) return fail(ctx, HPGV_ERR_INVALID, "task must be CHISQ or FISHER");
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) ||
        (max_lines > 0 && (!A1 || !A2 || !U1 || !U2 || !odds || !p || (task == HPGV_TASK_CHISQ && !chisq))))
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_text arguments");
    if (!n_sel || rows_cap < 0 || (max_lines > 0 && !sel) || (rows_cap > 0 && (!rows_out || rows_pitch < (size_t)ctx->assoc.n_samples)) || p_max != p_max)
        return fail(ctx, HPGV_ERR_INVALID, "bad assoc_select_text arguments");
    *n_lines = 0;
    *n_sel = 0;
    if (max_lines == 0) return HPGV_OK;
    std::vector<int32_t> own_status;             // (before the lease: queued copies into it end with the lease)
    HPGV_LEASE_SLOT(ctx)
    const bool fused = batch_fused_ok(ctx, ctx->assoc.n_samples);
    if (fused && task == HPGV_TASK_FISHER && (rc = logfact_check(ctx))) return rc;
    if (!status) { own_status.assign((size_t)max_lines, 0); status = own_status.data(); }
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_ASSOC, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S, !fused))) return rc;
    if (S.n == 0) { HIPCHK(ctx, hipStreamSynchronize(s->stream)); return HPGV_OK; }
    std::pair<const char *, size_t> p_at{nullptr, 0};
    if ((rc = assoc_finish(ctx, s, task, S, A1, A2, U1, U2, odds, chisq, p, &p_at))) return rc;
    return select_rows(ctx, s, S, ctx->assoc.n_samples, status, p_at.first, p_at.second, p_max, sel, rows_out, rows_pitch, rows_cap, n_sel);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_tdt(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
             int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_tdt(m_, gt, pitch, n_variants, is_x, t1, t2, odds, chisq, p))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->tdt.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_families has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!gt || !t1 || !t2 || !odds || !chisq || !p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad tdt arguments");
    if (pitch < (size_t)ctx->tdt.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->tdt.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_batch(ctx, s, batch_fused_ok(ctx, ctx->tdt.n_samples), HPGV_LAYOUT_TDT, ctx->tdt, gt, pitch, n_variants, is_x, &S))) return rc;
    return tdt_finish(ctx, s, S, t1, t2, odds, chisq, p);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_tdt_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                  uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *t1, int32_t *t2,
                  double *odds, double *chisq, double *p) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_tdt_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, t1, t2, odds, chisq, p))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->tdt.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_families has not been called");
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && (!t1 || !t2 || !odds || !chisq || !p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad tdt_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_TDT, ctx->tdt, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S,
                         !batch_fused_ok(ctx, ctx->tdt.n_samples)))) return rc;
    if (S.n == 0) { HIPCHK(ctx, hipStreamSynchronize(s->stream)); return HPGV_OK; }
    return tdt_finish(ctx, s, S, t1, t2, odds, chisq, p);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_stats_ex(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int32_t *counts8,
                  double *hwe_chi2, double *hwe_p, int32_t *sample_missing, int32_t *multi_idx,
                  int32_t *multi_table, int *n_multi) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_stats_ex(m_, gt, pitch, n_variants, counts8, hwe_chi2, hwe_p, sample_missing, multi_idx, multi_table, n_multi))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!gt || !counts8 || !hwe_chi2 || !hwe_p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad stats arguments");
    if (n_multi && *n_multi > 0 && (!multi_idx || !multi_table)) return fail(ctx, HPGV_ERR_INVALID, "multi-allelic outputs are NULL");
    if (pitch < (size_t)ctx->stats.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->stats.n_samples);
    const int cap = n_multi ? *n_multi : 0;
    if (n_multi) *n_multi = 0;
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    // with per-sample counters: everything in one pass of k_stats_all; without: the fused per-batch kernel.  Both read the
    // batch in place when it lies in page-locked memory
    const bool want_sm = sample_missing && ctx->stats.n_samples > 0;
    const bool one_pass = want_sm && stats_all_lds(ctx, false) != 0, batch_stats = !want_sm && batch_fused_ok(ctx, ctx->stats.n_samples);
    Staged S;
    if ((rc = stage_batch(ctx, s, one_pass || batch_stats, HPGV_LAYOUT_STATS, ctx->stats, gt, pitch, n_variants, nullptr, &S))) return rc;
    StatsAllOut O;
    O.counts8 = counts8; O.hwe_chi2 = hwe_chi2; O.hwe_p = hwe_p; O.sample_missing = sample_missing;
    return stats_finish(ctx, s, S, batch_stats, O, cap, multi_idx, multi_table, n_multi);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_stats(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int32_t *counts8,
               double *hwe_chi2, double *hwe_p) {
    return hpgv_stats_ex(ctx, gt, pitch, n_variants, counts8, hwe_chi2, hwe_p, nullptr, nullptr, nullptr, nullptr);
}

int hpgv_stats_groups(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, int32_t *counts8,
                      double *hwe_chi2, double *hwe_p) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_stats_groups(m_, gt, pitch, n_variants, counts8, hwe_chi2, hwe_p))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->sgroups.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_groups has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!gt || !counts8))) return fail(ctx, HPGV_ERR_INVALID, "bad stats group arguments");
    if ((hwe_chi2 == nullptr) != (hwe_p == nullptr)) return fail(ctx, HPGV_ERR_INVALID, "hwe_chi2 and hwe_p go together");
    if (pitch < (size_t)ctx->sgroups.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->sgroups.n_samples);
    if (n_variants == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    // the counters of every phenotype group from one pass over the batch (k_stats_all gathers every group's columns)
    const bool one_pass = ctx->stats.set && ctx->stats.n_samples == ctx->sgroups.n_samples && stats_all_lds(ctx, false) != 0;
    Staged S;
    if ((rc = stage_batch(ctx, s, one_pass, HPGV_LAYOUT_STATS_GROUPS, ctx->sgroups, gt, pitch, n_variants, nullptr, &S))) return rc;
    StatsAllOut O;
    O.group_counts8 = counts8; O.group_hwe_chi2 = hwe_chi2; O.group_hwe_p = hwe_p;
    return stats_finish(ctx, s, S, false, O, 0, nullptr, nullptr, nullptr);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_mendel(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                int32_t *errors, int32_t *child_errors) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_mendel(m_, gt, pitch, n_variants, is_x, errors, child_errors))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->mendel.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_pedigree has not been called");
    if (n_variants < 0 || (n_variants > 0 && !gt)) return fail(ctx, HPGV_ERR_INVALID, "bad mendel arguments");
    if (pitch < (size_t)ctx->mendel.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->mendel.n_samples);
    if (n_variants == 0 || (!errors && !child_errors)) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    const bool one_pass = ctx->stats.set && ctx->stats.n_samples == ctx->mendel.n_samples && stats_all_lds(ctx, true) != 0;
    Staged S;
    if ((rc = stage_batch(ctx, s, one_pass, HPGV_LAYOUT_MENDEL, ctx->mendel, gt, pitch, n_variants, is_x, &S))) return rc;
    StatsAllOut O;
    O.mendel_errors = errors; O.child_errors = child_errors;
    std::vector<int32_t> scratch;
    if (one_pass && !errors) { scratch.resize((size_t)n_variants); O.mendel_errors = scratch.data(); }      // k_stats_all's switch for the Mendel pass
    return stats_finish(ctx, s, S, false, O, 0, nullptr, nullptr, nullptr);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_stats_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                    uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *counts8, double *hwe_chi2,
                    double *hwe_p, int32_t *sample_missing, int32_t *multi_idx, int32_t *multi_table, int *n_multi,
                    int32_t *mendel_errors, int32_t *child_errors) {
    return hpgv_stats_text_groups(ctx, text, text_bytes, max_lines, n_lines, line_off, field_off, status, counts8, hwe_chi2, hwe_p,
                                  sample_missing, multi_idx, multi_table, n_multi, mendel_errors, child_errors, nullptr, nullptr, nullptr);
}

int hpgv_stats_text_groups(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                           uint64_t *line_off, uint32_t *field_off, int32_t *status, int32_t *counts8, double *hwe_chi2,
                           double *hwe_p, int32_t *sample_missing, int32_t *multi_idx, int32_t *multi_table, int *n_multi,
                           int32_t *mendel_errors, int32_t *child_errors, int32_t *group_counts8, double *group_hwe_chi2,
                           double *group_hwe_p) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_stats_text_groups(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, counts8, hwe_chi2, hwe_p, sample_missing, multi_idx, multi_table, n_multi, mendel_errors, child_errors, group_counts8, group_hwe_chi2, group_hwe_p))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && (!counts8 || !hwe_chi2 || !hwe_p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad stats_text arguments");
    if (n_multi && *n_multi > 0 && (!multi_idx || !multi_table)) return fail(ctx, HPGV_ERR_INVALID, "multi-allelic outputs are NULL");
    const bool want_mendel = mendel_errors || child_errors;
    if (want_mendel && (!ctx->mendel.set || ctx->mendel.n_samples != ctx->stats.n_samples))
        return fail(ctx, HPGV_ERR_STATE, "Mendelian errors need hpgv_set_pedigree over the same %d columns", ctx->stats.n_samples);
    if (group_counts8 && (!ctx->sgroups.set || ctx->sgroups.n_samples != ctx->stats.n_samples))
        return fail(ctx, HPGV_ERR_STATE, "per-group counters need hpgv_set_stats_groups over the same %d columns", ctx->stats.n_samples);
    if ((group_hwe_chi2 == nullptr) != (group_hwe_p == nullptr) || (group_hwe_chi2 && !group_counts8))
        return fail(ctx, HPGV_ERR_INVALID, "group_hwe_chi2 and group_hwe_p go together, with group_counts8");
    const int cap = n_multi ? *n_multi : 0;
    if (n_multi) *n_multi = 0;
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    const bool one_pass = stats_all_lds(ctx, want_mendel) != 0;   // LDS: the row window, a byte counter per column and per trio
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_STATS, ctx->stats, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S, !one_pass))) return rc;
    if (S.n == 0) { HIPCHK(ctx, hipStreamSynchronize(s->stream)); return HPGV_OK; }
    StatsAllOut O;
    O.counts8 = counts8; O.hwe_chi2 = hwe_chi2; O.hwe_p = hwe_p; O.sample_missing = sample_missing;
    O.mendel_errors = mendel_errors; O.child_errors = child_errors;
    O.group_counts8 = group_counts8; O.group_hwe_chi2 = group_hwe_chi2; O.group_hwe_p = group_hwe_p;
    return stats_finish(ctx, s, S, false, O, cap, multi_idx, multi_table, n_multi);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_epi_dataset(hpgv_ctx *ctx, const uint8_t *gt, size_t pitch, int n_variants, uint8_t *out) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_epi_dataset(m_, gt, pitch, n_variants, out))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!gt || !out))) return fail(ctx, HPGV_ERR_INVALID, "bad epi arguments");
    if (pitch < (size_t)ctx->assoc.n_samples) return fail(ctx, HPGV_ERR_INVALID, "pitch %zu < n_samples %d", pitch, ctx->assoc.n_samples);
    if (n_variants == 0 || ctx->nA + ctx->nU == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = stage_batch(ctx, s, false, HPGV_LAYOUT_EPI, ctx->assoc, gt, pitch, n_variants, nullptr, &S))) return rc;
    return epi_rows_out(ctx, s, S, out);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_epi_dataset_text(hpgv_ctx *ctx, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                          uint64_t *line_off, uint32_t *field_off, int32_t *status, uint8_t *out) {
    HPGV_ABI_TRY
    GROUP_DEAL_TEXT(ctx, text, hpgv_epi_dataset_text(m_, text, text_bytes, max_lines, n_lines, line_off, field_off, status, out))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (!n_lines || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !out))
        return fail(ctx, HPGV_ERR_INVALID, "bad epi_dataset_text arguments");
    *n_lines = 0;
    if (max_lines == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    Staged S;
    if ((rc = text_front(ctx, s, HPGV_LAYOUT_EPI, ctx->assoc, text, text_bytes, max_lines, n_lines, line_off, field_off, status, &S))) return rc;
    return epi_rows_out(ctx, s, S, out);
    HPGV_ABI_CATCH(ctx)
}

}  // extern "C"
