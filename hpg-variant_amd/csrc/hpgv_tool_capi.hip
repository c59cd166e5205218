// hpgv_tool_capi.hip -- C ABI of the tools' synchronous entry points (include/hpgv.h): the VCF text tokenizer, and
// association, TDT, statistics, Mendelian errors and the epistasis dataset on a host batch (hpgv_assoc, ...) or on a text
// (hpgv_assoc_text, ...).  An entry point checks its arguments, leases a slot, puts the matrix on the device -- a batch
// through batch_sources / stage_batch, a text through text_front -- and hands the result (a Staged) to its tool's back
// half, which is written once for both.
#include "hpgv_internal.h"
#include "hpgv_text_kernels.h"
#include "hpgv_text2_kernels.h"
#include "hpgv_batch_kernels.h"
#include "hpgv_inherit_kernels.h"

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

static int ensure_result_block(hpgv_ctx *ctx, Slot *s, size_t bytes) {
    if (s->res_cap >= bytes) return HPGV_OK;
    if (s->h_res) { (void)hipHostFree(s->h_res); s->h_res = nullptr; s->d_res = nullptr; s->res_cap = 0; }
    const size_t want = round_up(bytes + bytes / 2, 4096);
    HIPCHK(ctx, hipHostMalloc(&s->h_res, want, hipHostMallocDefault));
    HIPCHK(ctx, hipHostGetDevicePointer(&s->d_res, s->h_res, 0));
    s->res_cap = want;
    return HPGV_OK;
}

static bool batch_fused_ok(const hpgv_ctx *ctx, int n_samples) {
    return ctx->batch_fused && (size_t)n_samples + 32 <= (size_t)ctx->batch_lds_max;
}

// sources of a fused call: the caller's buffers as they are when the device can read them, the slot's copies otherwise
static int batch_sources(hpgv_ctx *ctx, Slot *s, const uint8_t *gt, size_t pitch, int n_variants, int n_samples, const uint8_t *is_x,
                         Staged *S) {
    int rc;
    const size_t bytes = (size_t)(n_variants - 1) * pitch + (size_t)n_samples;     // the last row need not be a whole pitch
    // page-locked rows are read in place by the kernel -- unless batch_copy asks for the copy engine first (it moves 2 MB in
    // 35 us where the kernel's own reads over the bus take 44; the kernel then runs on device memory)
    const void *src = ctx->batch_copy ? nullptr : mapped_view(gt, bytes);
    if (!src) {
        if ((rc = ensure(ctx, s, 0, bytes + 16))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s->buf[0], gt, bytes, hipMemcpyHostToDevice, s->stream));
        src = s->buf[0];
    }
    const void *x = nullptr;
    if (is_x) {
        x = mapped_view(is_x, (size_t)n_variants);
        if (!x) {
            if ((rc = ensure(ctx, s, 2, (size_t)n_variants))) return rc;
            HIPCHK(ctx, hipMemcpyAsync(s->buf[2], is_x, (size_t)n_variants, hipMemcpyHostToDevice, s->stream));
            x = s->buf[2];
        }
    }
    S->d_raw = (const uint8_t *)src; S->raw_pitch = pitch; S->d_isx = (const uint8_t *)x;
    S->n = n_variants; S->out_stride = (size_t)n_variants;
    return HPGV_OK;
}

// a batch on the device.  one_pass: for a kernel that reads the raw rows itself (batch_sources); else for the kernel chain:
// raw rows and is_x copied to the slot, the rows laid out for the tool (`which`)
// slot buffers: 0 raw gt, 1 laid-out gt, 2 is_x, 3 counts, 4 doubles (3n), 5 int SoA
static int stage_batch(hpgv_ctx *ctx, Slot *s, bool one_pass, int which, const Layout &L, const uint8_t *gt, size_t pitch,
                       int n_variants, const uint8_t *is_x, Staged *S) {
    int rc;
    if (one_pass) return batch_sources(ctx, s, gt, pitch, n_variants, L.n_samples, is_x, S);
    if ((rc = ensure(ctx, s, 0, (size_t)n_variants * pitch))) return rc;
    if ((rc = ensure(ctx, s, 1, (size_t)n_variants * L.pitch))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(s->buf[0], gt, (size_t)n_variants * pitch, hipMemcpyHostToDevice, s->stream));
    if (is_x) {
        if ((rc = ensure(ctx, s, 2, (size_t)n_variants))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(s->buf[2], is_x, (size_t)n_variants, hipMemcpyHostToDevice, s->stream));
        S->d_isx = (const uint8_t *)s->buf[2];
    }
    S->d_raw = (const uint8_t *)s->buf[0]; S->raw_pitch = pitch; S->d_laid = (const uint8_t *)s->buf[1]; S->which = which;
    S->n = n_variants; S->out_stride = (size_t)n_variants;
    return hpgv_layout_dev(ctx, which, S->d_raw, pitch, n_variants, (uint8_t *)s->buf[1], s->stream);
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
    int rc;
    const int n_variants = S.n;
    const size_t n = (size_t)n_variants, group_stride = S.out_stride;
    const int ns = ctx->stats.n_samples;
    const bool want_mendel = O.mendel_errors || O.child_errors;
    const size_t ng = O.group_counts8 ? ctx->sg_off.size() : 0, nt = want_mendel ? (size_t)ctx->mendel_trios : 0;
    const size_t rec_bytes = (1 + ng) * n * sizeof(hpgv::BatchStatsRec);
    if ((rc = ensure_result_block(ctx, s, rec_bytes + n * sizeof(int32_t) + 64))) return rc;
    const bool want_sm = O.sample_missing && ns > 0, want_ce = O.child_errors && nt > 0;
    if ((rc = ensure(ctx, s, 3, ((size_t)ns + nt + 16) * sizeof(int32_t)))) return rc;
    int32_t *d_sm = (int32_t *)s->buf[3], *d_ce = d_sm + ns;
    if (want_sm || want_ce) HIPCHK(ctx, hipMemsetAsync(d_sm, 0, ((size_t)ns + nt) * sizeof(int32_t), s->stream));
    hpgv::StatsAllArgs A;
    memset(&A, 0, sizeof A);
    A.src = S.d_raw; A.src_pitch = S.raw_pitch; A.n_variants = n_variants; A.n_samples = ns;
    A.is_x = S.d_isx;
    A.out = (hpgv::BatchStatsRec *)s->d_res;
    A.sample_missing = want_sm ? d_sm : nullptr;
    if (want_mendel) {
        A.mendel_cols = ctx->mendel.d_col_of_pos; A.pchunks = ctx->mendel_pchunks; A.n_trios = ctx->mendel_trios;
        A.luts = ctx->mendel_luts; A.male_plane = ctx->d_mendel_male;
        A.mendel_errors = O.mendel_errors ? (int32_t *)((char *)s->d_res + rec_bytes) : nullptr;
        A.child_errors = want_ce ? d_ce : nullptr;
    }
    if (ng) {
        A.group_cols = ctx->sgroups.d_col_of_pos; A.n_groups = (int)ng;
        A.group_chunk0 = ctx->d_sg_chunks; A.group_chunks = ctx->d_sg_chunks + ng;
        A.group_out = (hpgv::BatchStatsRec *)s->d_res + n;
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
    if (!ctx->stats_all2 || hpgv_launch_stats_all2(ctx, A, &s->cnt_buf, &s->cnt_cap, s->stream) != 0) {
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
    const hpgv::BatchStatsRec *r = (const hpgv::BatchStatsRec *)s->h_res;
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
    if (O.mendel_errors) memcpy(O.mendel_errors, (const char *)s->h_res + rec_bytes, n * sizeof(int32_t));
    if (want_sm) for (int j = 0; j < ns; ++j) O.sample_missing[j] += acc[(size_t)j];
    if (want_ce) for (size_t t = 0; t < nt; ++t) O.child_errors[t] += acc[(size_t)ns + t];
    return HPGV_OK;
}

// the fused kernel of one tool over a staged matrix: raw rows (read in place from page-locked memory, or the tokenizer's)
// -> layout in registers -> counts -> statistics -> packed records of rec_bytes each.  The caller has filled the tool's
// fields of A (and n_samples); when this returns the records lie in the slot's page-locked block, s->h_res
template <int KIND>
static int launch_batch(hpgv_ctx *ctx, Slot *s, const Staged &S, hpgv::BatchArgs &A, size_t rec_bytes) {
    if (const int rc = ensure_result_block(ctx, s, (size_t)S.n * rec_bytes)) return rc;
    A.src = S.d_raw; A.src_pitch = S.raw_pitch; A.n_variants = S.n; A.is_x = S.d_isx;
    A.out = s->d_res;
    const size_t lds = ((size_t)A.n_samples + 15 + 15) / 16 * 16 + 16;
    hipLaunchKernelGGL((hpgv::k_batch<KIND>), dim3((unsigned)A.n_variants), dim3(256), lds, s->stream, A);
    if (const int rc = [&] { HIPCHK(ctx, hipGetLastError()); return (int)HPGV_OK; }()) { (void)hipStreamSynchronize(s->stream); return rc; }
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

// ---- the tools' back halves: from a staged matrix to the caller's arrays, written once for a batch and a text -------------

// chi-square or Fisher per variant.  A text that skipped the layout is counted by k_assoc_rows where that kernel takes
// the cohort; any matrix that skipped it goes through the fused kernel; a laid-out one through the scans' kernel chain
static int assoc_finish(hpgv_ctx *ctx, Slot *s, int task, const Staged &S, int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                        double *odds, double *chisq, double *p) {
    int rc;
    const int nv = S.n;
    const size_t n = (size_t)nv;
    const bool chi = task == HPGV_TASK_CHISQ, rows = !S.d_laid && S.text && ctx->assoc_rows;
    if (S.d_laid || rows) {
        if ((rc = ensure(ctx, s, 3, n * 16))) return rc;
        if ((rc = ensure(ctx, s, 4, n * 3 * sizeof(double)))) return rc;
    }
    int32_t *d_counts = (int32_t *)s->buf[3];
    double *d_odds = (double *)s->buf[4], *d_chisq = d_odds + n, *d_p = d_odds + 2 * n;
    auto statistics = [&] {
        return chi ? hpgv_assoc_chisq_dev(ctx, d_counts, nv, d_odds, d_chisq, d_p, s->stream)
                   : hpgv_assoc_fisher_dev(ctx, d_counts, nv, d_odds, d_p, s->stream);
    };
    if (rows) {
        // the raw matrix read once by threads that own columns (k_assoc_rows), then the scans' own statistics kernels
        if ((rc = ensure_result_block(ctx, s, n * 40 + 64))) return rc;
        if (hpgv_launch_assoc_rows(ctx, S.d_raw, S.raw_pitch, nv, S.d_isx, d_counts, s->stream) == 0) {
            HIPCHK(ctx, hipGetLastError());
            if ((rc = statistics())) { (void)hipStreamSynchronize(s->stream); return rc; }
            // results come back through the slot's page-locked block (one copy each at the bus rate), then into the caller's arrays
            char *h = (char *)s->h_res;
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
    if (!S.d_laid) {
        // one kernel; the only other work of the call is unpacking its records
        hpgv::BatchArgs A;
        memset(&A, 0, sizeof A);
        A.n_samples = ctx->assoc.n_samples;
        A.col_of_pos = ctx->assoc.d_col_of_pos; A.chunks = ctx->assoc.chunks; A.chunksA = ctx->chunksA;
        A.lf = ctx->d_lf; A.rel_cut = pow(10.0, -(double)ctx->fisher_cut_exp);
        rc = chi ? launch_batch<hpgv::BATCH_CHISQ>(ctx, s, S, A, sizeof(hpgv::BatchAssocRec))
                 : launch_batch<hpgv::BATCH_FISHER>(ctx, s, S, A, sizeof(hpgv::BatchAssocRec));
        if (rc) return rc;
        const hpgv::BatchAssocRec *r = (const hpgv::BatchAssocRec *)s->h_res;
        for (size_t i = 0; i < n; ++i) {
            A1[i] = r[i].A1; A2[i] = r[i].A2; U1[i] = r[i].U1; U2[i] = r[i].U2;
            odds[i] = r[i].odds; p[i] = r[i].p;
        }
        if (chi) for (size_t i = 0; i < n; ++i) chisq[i] = r[i].chisq;
        return HPGV_OK;
    }
    if ((rc = ensure(ctx, s, 5, n * 4 * sizeof(int32_t)))) return rc;      // (a text's status array has been copied out of it: same stream)
    int32_t *d_soa = (int32_t *)s->buf[5];
    if ((rc = hpgv_assoc_scan_dev(ctx, S.d_laid, nv, S.d_isx, d_counts, s->stream))) return rc;
    if ((rc = statistics())) return rc;
    hipLaunchKernelGGL(hpgv::k_counts_to_soa, dim3((nv + 255) / 256), dim3(256), 0, s->stream,
                       (const int4 *)d_counts, nv, d_soa, d_soa + n, d_soa + 2 * n, d_soa + 3 * n);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(A1, d_soa, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(A2, d_soa + n, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(U1, d_soa + 2 * n, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(U2, d_soa + 3 * n, n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(odds, d_odds, n * 8, hipMemcpyDeviceToHost, s->stream));
    if (chi) HIPCHK(ctx, hipMemcpyAsync(chisq, d_chisq, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(p, d_p, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

static int tdt_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, int32_t *t1, int32_t *t2, double *odds, double *chisq, double *p) {
    int rc;
    const int nv = S.n;
    const size_t n = (size_t)nv;
    if (!S.d_laid) {
        hpgv::BatchArgs A;
        memset(&A, 0, sizeof A);
        const hpgv::TdtPlan &P = ctx->tdt_plan;
        A.n_samples = ctx->tdt.n_samples;
        A.col_of_pos = ctx->tdt.d_col_of_pos; A.chunks = ctx->tdt.chunks;
        A.pchunks = P.pchunks; A.p16 = P.p16; A.n_slow = P.n_slow_families; A.slow_base = P.slow_base; A.luts = P.luts;
        A.male_plane = P.d_male_plane; A.slow_off = P.d_slow_off; A.slow_male = P.d_slow_male;
        if ((rc = launch_batch<hpgv::BATCH_TDT>(ctx, s, S, A, sizeof(hpgv::BatchTdtRec)))) return rc;
        const hpgv::BatchTdtRec *r = (const hpgv::BatchTdtRec *)s->h_res;
        for (size_t i = 0; i < n; ++i) { t1[i] = r[i].t1; t2[i] = r[i].t2; odds[i] = r[i].odds; chisq[i] = r[i].chisq; p[i] = r[i].p; }
        return HPGV_OK;
    }
    if ((rc = ensure(ctx, s, 3, n * 8))) return rc;
    if ((rc = ensure(ctx, s, 4, n * 3 * sizeof(double)))) return rc;
    int32_t *d_tu = (int32_t *)s->buf[3];
    double *d_odds = (double *)s->buf[4], *d_chisq = d_odds + n, *d_p = d_odds + 2 * n;
    if ((rc = hpgv_tdt_scan_dev(ctx, S.d_laid, nv, S.d_isx, d_tu, s->stream))) return rc;
    if ((rc = hpgv_tdt_stats_dev(ctx, d_tu, nv, d_odds, d_chisq, d_p, s->stream))) return rc;
    std::vector<int32_t> tu(2 * n);
    HIPCHK(ctx, hipMemcpyAsync(tu.data(), d_tu, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(odds, d_odds, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(chisq, d_chisq, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(p, d_p, n * 8, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < n; ++i) { t1[i] = tu[2 * i]; t2[i] = tu[2 * i + 1]; }
    return HPGV_OK;
}

// the staged rows in layout `which`: as they are when they were laid out for it, else laid out again from the raw matrix
// (what buf[1] held has been consumed by then: same stream)
static int laid_as(hpgv_ctx *ctx, Slot *s, const Staged &S, int which, const Layout &L, const uint8_t **d_out) {
    *d_out = S.d_laid;
    if (S.which == which) return HPGV_OK;
    if (const int rc = ensure(ctx, s, 1, (size_t)S.n * L.pitch + 16)) return rc;
    *d_out = (const uint8_t *)s->buf[1];
    return hpgv_layout_dev(ctx, which, S.d_raw, S.raw_pitch, S.n, (uint8_t *)s->buf[1], s->stream);
}

// the statistics of a laid-out matrix by the scans' kernels, each output of O that is asked for: counters and
// Hardy-Weinberg with the per-sample missing counts, then Mendelian errors, then the counters of every phenotype group
static int stats_chain(hpgv_ctx *ctx, Slot *s, const Staged &S, const StatsAllOut &O) {
    int rc;
    const int nv = S.n, ns = ctx->stats.n_samples;
    const size_t n = (size_t)nv;
    std::vector<int32_t> sm, ce;
    if (O.counts8) {
        if ((rc = ensure(ctx, s, 3, n * 32))) return rc;
        if ((rc = ensure(ctx, s, 4, n * 2 * sizeof(double) + 64))) return rc;
        int32_t *d_c8 = (int32_t *)s->buf[3];
        double *d_chi2 = (double *)s->buf[4], *d_p = d_chi2 + n;
        if ((rc = hpgv_stats_scan_dev(ctx, S.d_laid, nv, d_c8, s->stream))) return rc;
        if ((rc = hpgv_stats_hwe_dev(ctx, d_c8, nv, d_chi2, d_p, s->stream))) return rc;
        if (O.sample_missing && ns > 0) {                            // (a text's status array has been copied out of buf[5])
            if ((rc = ensure(ctx, s, 5, (size_t)ns * sizeof(int32_t)))) return rc;
            int32_t *d_sm = (int32_t *)s->buf[5];
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
        const uint8_t *d_gt;
        if ((rc = laid_as(ctx, s, S, HPGV_LAYOUT_MENDEL, ctx->mendel, &d_gt))) return rc;
        if ((rc = ensure(ctx, s, 6, (n + nt) * sizeof(int32_t) + 64))) return rc;   // (a text's line offsets have been copied out of it)
        int32_t *d_err = (int32_t *)s->buf[6], *d_child = d_err + n;
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
        if (O.counts8) HIPCHK(ctx, hipStreamSynchronize(s->stream));   // the copies out of buf[3] / buf[4] above are done before their reuse
        const uint8_t *d_gt;
        if ((rc = laid_as(ctx, s, S, HPGV_LAYOUT_STATS_GROUPS, ctx->sgroups, &d_gt))) return rc;
        if ((rc = ensure(ctx, s, 3, ng * n * 32 + 64))) return rc;
        if ((rc = ensure(ctx, s, 4, ng * n * 2 * sizeof(double) + 64))) return rc;
        int32_t *d_g8 = (int32_t *)s->buf[3];
        double *d_ghw = (double *)s->buf[4];
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
// them; *n_multi says how many there are).  Runs after the call's other results are back: the slot's buf[3] is free
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
        if (const int e = ensure(ctx, s, 3, (size_t)m * 257 * sizeof(int32_t))) return e;
        int32_t *d_idx = (int32_t *)s->buf[3], *d_tab = d_idx + m;
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
        A.col_of_pos = ctx->stats.d_col_of_pos; A.chunks = ctx->stats.chunks;
        if ((rc = launch_batch<hpgv::BATCH_STATS>(ctx, s, S, A, sizeof(hpgv::BatchStatsRec)))) return rc;
        const hpgv::BatchStatsRec *r = (const hpgv::BatchStatsRec *)s->h_res;
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

/* ---- text staging ------------------------------------------------------------ */

// (hpgv_inflate_blocks_dev: hpgv_inflate_capi.hip)

int hpgv_tokenize_dev(hpgv_ctx *ctx, const char *d_text, size_t text_bytes, int n_samples, int strict,
                      int max_lines, int *d_n_lines, uint64_t *d_line_off, uint32_t *d_field_off,
                      uint8_t *d_gt, size_t pitch, uint8_t *d_is_x, int32_t *d_status, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_samples < 0 || max_lines < 0 || !d_n_lines || (text_bytes > 0 && !d_text) ||
        (max_lines > 0 && !d_gt) || pitch < (size_t)n_samples)
        return fail(ctx, HPGV_ERR_INVALID, "bad tokenize arguments");
    if (text_bytes > ((size_t)1 << 40)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "text buffer too large for one call");
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    // a window of text the bgzip decoder left with its tile records (hpgv_text_alias_tiles): tokenized on the decoder's tile grid,
    // from the start of the tile the window begins in (grid_skip bytes in front of the window: the tail of the line before it)
    hpgv_ctx::TextTiles TT = {nullptr, nullptr, nullptr, 0};
    bool grid = false;
    size_t grid_t0 = 0, grid_skip = 0;
    if (ctx->tokenizer_tiles == 1 && ctx->decode_tiles && text_bytes > 0 && tiles_of_device_text(ctx, d_text, &TT)) {
        const size_t a = (size_t)(d_text - TT.d_base), e = a + text_bytes;
        if ((e - 1) / hpgv::TOK2_TILE < TT.n_tiles) {
            grid = true; grid_t0 = a / hpgv::TOK2_TILE; grid_skip = a - grid_t0 * hpgv::TOK2_TILE;
            d_text -= grid_skip; text_bytes += grid_skip;
        }
    }
    const size_t n_blocks = (text_bytes + hpgv::TOK_TILE - 1) / hpgv::TOK_TILE;
    if (n_blocks > 0x7FFFFFFFu) return fail(ctx, HPGV_ERR_UNSUPPORTED, "text buffer too large for one call");
    hpgv_ctx::TokScratch *ts = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->tok_mu);
        for (auto *t : ctx->tok_scratch) if (t->stream == st) ts = t;
        if (!ts) { ts = new hpgv_ctx::TokScratch(); ts->stream = st; ctx->tok_scratch.push_back(ts); }
    }
    // from here on `ts` is only touched by calls on stream `st`, which the caller does not issue concurrently
    // scratch per tile: the newline counts of the three-sweep form (4 B), or the tile records and tile states of the
    // tile-parallel form (16 B + 16 B)
    const size_t scratch_ints = (n_blocks + 1) * 8 * (hpgv::TOK_TILE / hpgv::TOK2_TILE > 1 ? hpgv::TOK_TILE / hpgv::TOK2_TILE : 1) + 64;            // (+ the one-sweep form's 64-byte head and the records of a text of a few bytes)
    if (ts->blocks_cap < scratch_ints) {
        if (ts->d_blocks) { HIPCHK(ctx, hipStreamSynchronize(st)); (void)hipFree(ts->d_blocks); ts->d_blocks = nullptr; ts->blocks_cap = 0; }
        HIPCHK(ctx, hipMalloc(&ts->d_blocks, scratch_ints * sizeof(int)));
        ts->blocks_cap = scratch_ints;
    }
    unsigned long long *line_off = (unsigned long long *)d_line_off;
    if (!line_off) {                                   // caller does not want the offsets: use scratch
        if (ts->line_cap < (size_t)max_lines + 2) {
            if (ts->d_line_off) { HIPCHK(ctx, hipStreamSynchronize(st)); (void)hipFree(ts->d_line_off); ts->d_line_off = nullptr; ts->line_cap = 0; }
            HIPCHK(ctx, hipMalloc(&ts->d_line_off, ((size_t)max_lines + 2) * sizeof(unsigned long long)));
            ts->line_cap = (size_t)max_lines + 2;
        }
        line_off = ts->d_line_off;
    }
    if (ctx->tokenizer_tiles) {
        // two sweeps of the text: tile records, tile states, then one workgroup per tile parses (hpgv_text2_kernels.h)
        const size_t n_tiles = (text_bytes + hpgv::TOK2_TILE - 1) / hpgv::TOK2_TILE;      // 2 KiB tiles
        hpgv::TokAgg *agg = (hpgv::TokAgg *)ts->d_blocks;
        hpgv::TokPre *pre = (hpgv::TokPre *)(agg + n_tiles + 1);
        const int n_groups = (int)((n_tiles + hpgv::TOK_SCAN_THREADS - 1) / hpgv::TOK_SCAN_THREADS);
        // the groups' totals and the per-line "parse again" flags live behind the line offsets' scratch
        const size_t extra = ((size_t)n_groups + 2) * sizeof(hpgv::TokState) + ((size_t)max_lines + 2) * sizeof(int);
        if (ts->extra_cap < extra) {
            if (ts->d_extra) { HIPCHK(ctx, hipStreamSynchronize(st)); (void)hipFree(ts->d_extra); ts->d_extra = nullptr; ts->extra_cap = 0; }
            HIPCHK(ctx, hipMalloc(&ts->d_extra, extra + extra / 4));
            ts->extra_cap = extra + extra / 4;
        }
        hpgv::TokState *gtot = (hpgv::TokState *)ts->d_extra;
        int *redo = (int *)(gtot + n_groups + 2), *redo_n = redo + max_lines + 1;      // the list of lines to parse again, its length
        const unsigned redo_grid = (unsigned)(max_lines < 1024 ? max_lines : 1024);
#ifdef HPGV_ABLATION
        if (ctx->tokenizer_tiles >= 2 && n_tiles > 0 && max_lines > 0) {
            // ONE sweep: count, scan and parse in one kernel, the segments' start states by look-back (k_tok_parse3).  The
            // records, the ticket and the error flag share the tile scratch (zeroed per call: 16 bytes per 32 KiB of text).
            const size_t n_seg = (text_bytes + hpgv::TOK3_SEG - 1) / hpgv::TOK3_SEG;
            unsigned *tk = (unsigned *)ts->d_blocks;
            int *err = (int *)ts->d_blocks + 1;
            redo_n = (int *)ts->d_blocks + 2;                          // (zeroed with the records)
            const size_t n_sup = (n_seg + hpgv::TOK3_SUPER - 1) / hpgv::TOK3_SUPER;
            hpgv::TokRec *rec = (hpgv::TokRec *)((char *)ts->d_blocks + 64), *sup = rec + n_seg;
            HIPCHK(ctx, hipMemsetAsync(ts->d_blocks, 0, 64 + (n_seg + n_sup) * sizeof(hpgv::TokRec), st));
            hipLaunchKernelGGL(hpgv::k_tok_parse3, dim3((unsigned)n_seg), dim3(256), 0, st, d_text, text_bytes, rec, sup, tk, err, d_n_lines,
                               max_lines, n_samples, strict, d_gt, pitch, d_is_x, line_off, d_field_off, d_status, redo, redo_n);
            hipLaunchKernelGGL(hpgv::k_tok_finish, dim3(1), dim3(1), 0, st, (const int *)err, d_n_lines);
            hipLaunchKernelGGL(hpgv::k_tok_parse_listed, dim3(redo_grid), dim3(256), 0, st, d_text, line_off,
                               (const int *)d_n_lines, max_lines, n_samples, strict, d_gt, pitch, d_is_x, d_field_off, d_status, (const int *)redo, (const int *)redo_n);
            HIPCHK(ctx, hipGetLastError());
            return HPGV_OK;
        }
#endif
        if (grid && n_tiles > 0) {
            // the decoder's records serve every tile but the window's last, which is counted again up to the window's end
            // (and the bytes in front of the window, for the number of lines that end there)
            const size_t lt = n_tiles - 1;
            hipLaunchKernelGGL(hpgv::k_tok_count2, dim3(1), dim3(256), 0, st, d_text + lt * hpgv::TOK2_TILE, text_bytes - lt * hpgv::TOK2_TILE, 1, agg);
            if (grid_skip) hipLaunchKernelGGL(hpgv::k_tok_count2, dim3(1), dim3(256), 0, st, d_text, grid_skip, 1, agg + 1);
            hipLaunchKernelGGL(hpgv::k_tok_scan2a_grid, dim3((unsigned)n_groups), dim3(hpgv::TOK_SCAN_THREADS), 0, st, (const hpgv::TokAgg2 *)TT.d_tiles, (long)grid_t0,
                               (const hpgv::TokAgg *)agg, d_text, text_bytes, (int)n_tiles, pre, gtot);
        } else if (n_tiles > 0) {
            hipLaunchKernelGGL(hpgv::k_tok_count2, dim3((unsigned)((n_tiles + hpgv::TOK2_COUNT_TILES - 1) / hpgv::TOK2_COUNT_TILES)), dim3(256), 0, st, d_text, text_bytes, (int)n_tiles, agg);
            hipLaunchKernelGGL(hpgv::k_tok_scan2a, dim3((unsigned)n_groups), dim3(hpgv::TOK_SCAN_THREADS), 0, st, (const hpgv::TokAgg *)agg, (int)n_tiles, pre, gtot);
        }
        hipLaunchKernelGGL(hpgv::k_tok_scan2b, dim3((unsigned)(n_groups > 0 ? n_groups : 1)), dim3(hpgv::TOK_SCAN_THREADS), 0, st, pre, (int)n_tiles, gtot, n_groups,
                           d_text, text_bytes, d_n_lines, line_off, max_lines, redo_n, grid_skip ? (const hpgv::TokAgg *)(agg + 1) : (const hpgv::TokAgg *)nullptr);
        if (n_tiles > 0 && max_lines > 0) {
            hipLaunchKernelGGL(hpgv::k_tok_parse2, dim3((unsigned)n_tiles), dim3(hpgv::TOK2_THREADS), 0, st, d_text, text_bytes, (const hpgv::TokPre *)pre,
                               max_lines, n_samples, strict, d_gt, pitch, d_is_x, line_off, d_field_off, d_status, redo, redo_n, (int)grid_skip);
            // the lines whose FORMAT does not begin with GT (listed by the thread that read it): once more, line by line
            hipLaunchKernelGGL(hpgv::k_tok_parse_listed, dim3(redo_grid), dim3(256), 0, st, d_text, line_off,
                               (const int *)d_n_lines, max_lines, n_samples, strict, d_gt, pitch, d_is_x, d_field_off, d_status, (const int *)redo, (const int *)redo_n);
        }
        if (grid_skip)                                               // positions counted from the first tile's start: back to the window's
            hipLaunchKernelGGL(hpgv::k_tok_grid_finish, dim3((unsigned)((max_lines + 256) / 256)), dim3(256), 0, st, line_off, (const int *)d_n_lines, max_lines, (unsigned)grid_skip);
        HIPCHK(ctx, hipGetLastError());
        return HPGV_OK;
    }
#ifndef HPGV_ABLATION
    return fail(ctx, HPGV_ERR_UNSUPPORTED, "the line-by-line tokenizer is an ablation build's");
#else
    if (n_blocks > 0)
        hipLaunchKernelGGL(hpgv::k_tok_count, dim3((unsigned)n_blocks), dim3(256), 0, st, d_text, text_bytes, ts->d_blocks);
    hipLaunchKernelGGL(hpgv::k_tok_scan, dim3(1), dim3(hpgv::TOK_SCAN_THREADS), 0, st, ts->d_blocks, (int)n_blocks, d_text, text_bytes,
                       d_n_lines, line_off, max_lines);
    if (n_blocks > 0)
        hipLaunchKernelGGL(hpgv::k_tok_mark, dim3((unsigned)n_blocks), dim3(256), 0, st, d_text, text_bytes,
                           (const int *)ts->d_blocks, line_off, max_lines);
    else
        HIPCHK(ctx, hipMemsetAsync(line_off, 0, sizeof(unsigned long long), st));
    if (max_lines > 0)
        hipLaunchKernelGGL(hpgv::k_tok_parse, dim3((unsigned)max_lines), dim3(256), 0, st, d_text, line_off,
                           (const int *)d_n_lines, max_lines, n_samples, strict, d_gt, pitch, d_is_x, d_field_off, d_status);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
#endif
    HPGV_ABI_CATCH(ctx)
}

int hpgv_tokenize(hpgv_ctx *ctx, const char *text, size_t text_bytes, int n_samples, int strict, int max_lines,
                  int *n_lines, uint64_t *line_off, uint32_t *field_off, uint8_t *gt, size_t pitch,
                  uint8_t *is_x, int32_t *status) {
    GROUP_DEAL(ctx, hpgv_tokenize(m_, text, text_bytes, n_samples, strict, max_lines, n_lines, line_off, field_off, gt, pitch, is_x, status))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!n_lines || n_samples < 0 || max_lines < 0 || (text_bytes > 0 && !text) || (max_lines > 0 && !gt) ||
        pitch < (size_t)n_samples)
        return fail(ctx, HPGV_ERR_INVALID, "bad tokenize arguments");
    HPGV_LEASE_SLOT(ctx)
    const size_t ml = (size_t)max_lines;
    if ((rc = ensure(ctx, s, 0, text_bytes + 16))) return rc;
    if ((rc = ensure(ctx, s, 1, ml * pitch + 16))) return rc;
    if ((rc = ensure(ctx, s, 2, ml + 16))) return rc;
    if ((rc = ensure(ctx, s, 3, (ml + 2) * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(ctx, s, 4, ml * 10 * sizeof(uint32_t) + 16))) return rc;
    if ((rc = ensure(ctx, s, 5, ml * sizeof(int32_t) + 16))) return rc;
    if ((rc = ensure(ctx, s, 6, 16))) return rc;
    if (text_bytes) HIPCHK(ctx, hipMemcpyAsync(s->buf[0], text, text_bytes, hipMemcpyHostToDevice, s->stream));
    if ((rc = hpgv_tokenize_dev(ctx, (const char *)s->buf[0], text_bytes, n_samples, strict, max_lines, (int *)s->buf[6],
                                (uint64_t *)s->buf[3], (uint32_t *)s->buf[4], (uint8_t *)s->buf[1], pitch,
                                (uint8_t *)s->buf[2], (int32_t *)s->buf[5], s->stream))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(n_lines, s->buf[6], sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    if (*n_lines < 0) {                                             // the one-sweep tokenizer gave up a look-back: the two-sweep kernels from now on
        ctx->tokenizer_tiles = 1;
        if ((rc = hpgv_tokenize_dev(ctx, (const char *)s->buf[0], text_bytes, n_samples, strict, max_lines, (int *)s->buf[6],
                                    (uint64_t *)s->buf[3], (uint32_t *)s->buf[4], (uint8_t *)s->buf[1], pitch,
                                    (uint8_t *)s->buf[2], (int32_t *)s->buf[5], s->stream))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(n_lines, s->buf[6], sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
    }
    const size_t nl = (size_t)(*n_lines < max_lines ? *n_lines : max_lines);
    if (nl) {
        HIPCHK(ctx, hipMemcpyAsync(gt, s->buf[1], nl * pitch, hipMemcpyDeviceToHost, s->stream));
        if (is_x) HIPCHK(ctx, hipMemcpyAsync(is_x, s->buf[2], nl, hipMemcpyDeviceToHost, s->stream));
        if (field_off) HIPCHK(ctx, hipMemcpyAsync(field_off, s->buf[4], nl * 10 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        if (status) HIPCHK(ctx, hipMemcpyAsync(status, s->buf[5], nl * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    }
    if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, s->buf[3], (nl + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

}  // extern "C"

// shared front half of the *_text entry points: text -> device, tokenize, lay out.
// slot buffers: 0 text, 1 laid-out gt, 2 is_x, 3 tallies, 4 doubles, 5 SoA ints / status,
// 6 {n_lines, line_off..., field_off...}, 7 raw gt (VCF order)
int text_front(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const char *text, size_t text_bytes,
               int max_lines, int *n_lines, uint64_t *line_off, uint32_t *field_off, int32_t *status,
               Staged *S, bool final_layout) {
    int rc;
    const size_t ml = (size_t)max_lines;
    const size_t raw_pitch = raw_pitch_of(L.n_samples);
    const size_t off_lines = 16, off_fields = off_lines + (ml + 2) * sizeof(uint64_t);
    if ((rc = ensure(ctx, s, 0, text_bytes + 16))) return rc;
    if ((rc = ensure(ctx, s, 7, ml * raw_pitch + 16))) return rc;
    if ((rc = ensure(ctx, s, 1, ml * L.pitch + 16))) return rc;
    if ((rc = ensure(ctx, s, 2, ml + 16))) return rc;
    if ((rc = ensure(ctx, s, 5, ml * 4 * sizeof(int32_t) + 16))) return rc;
    if ((rc = ensure(ctx, s, 6, off_fields + ml * 10 * sizeof(uint32_t) + 16))) return rc;
    char *meta = (char *)s->buf[6];
    const char *d_src = text_on_device(ctx, text);                  // hpgv_text_alias: the text is on the device already
    const bool aliased = d_src != nullptr;
    if (!d_src) {
        if (text_bytes) HIPCHK(ctx, hipMemcpyAsync(s->buf[0], text, text_bytes, hipMemcpyHostToDevice, s->stream));
        d_src = (const char *)s->buf[0];
    }
    // the raw matrix keeps half-called genotypes ("./1"): the record filters count alleles as the stats tool does;
    // the strict layouts (assoc, tdt, epi) turn every not fully called genotype into "missing" on their way in
    if ((rc = hpgv_tokenize_dev(ctx, d_src, text_bytes, L.n_samples, 0,
                                max_lines, (int *)meta, (uint64_t *)(meta + off_lines), (uint32_t *)(meta + off_fields),
                                (uint8_t *)s->buf[7], raw_pitch, (uint8_t *)s->buf[2], (int32_t *)s->buf[5], s->stream))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(n_lines, meta, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    if (*n_lines < 0) {                                             // the one-sweep tokenizer gave up a look-back: the two-sweep kernels from now on
        ctx->tokenizer_tiles = 1;
        if ((rc = hpgv_tokenize_dev(ctx, d_src, text_bytes, L.n_samples, 0,
                                    max_lines, (int *)meta, (uint64_t *)(meta + off_lines), (uint32_t *)(meta + off_fields),
                                    (uint8_t *)s->buf[7], raw_pitch, (uint8_t *)s->buf[2], (int32_t *)s->buf[5], s->stream))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(n_lines, meta, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
    }
    const int nl = *n_lines < max_lines ? *n_lines : max_lines;
    S->text = true;
    S->d_raw = (const uint8_t *)s->buf[7]; S->raw_pitch = raw_pitch; S->d_isx = (const uint8_t *)s->buf[2];
    S->n = nl; S->out_stride = ml;
    if (nl == 0) return HPGV_OK;
    if (status) HIPCHK(ctx, hipMemcpyAsync(status, s->buf[5], (size_t)nl * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (aliased) {
        // the text is on the device only: the caller's host buffer gets the line heads (CHROM .. FORMAT, all it reads for its
        // result records) and line_off refers to them
        const int hb = (nl + 1023) / 1024;                          // workgroups of 1024 lines
        const size_t off_heads = (((size_t)nl + 2 + (size_t)hb + 1) * sizeof(uint64_t) + 15) / 16 * 16;
        if ((rc = ensure(ctx, s, 0, text_bytes + off_heads + 64))) return rc;
        unsigned long long *d_head_off = (unsigned long long *)s->buf[0], *d_block = d_head_off + (size_t)nl + 2;
        char *d_heads = (char *)s->buf[0] + off_heads;
        hipLaunchKernelGGL(hpgv::k_head_sums, dim3((unsigned)hb), dim3(1024), 0, s->stream, (const unsigned long long *)(meta + off_lines),
                           (const uint32_t *)(meta + off_fields), nl, d_block);
        hipLaunchKernelGGL(hpgv::k_head_bases, dim3(1), dim3(1024), 0, s->stream, d_block, hb);
        hipLaunchKernelGGL(hpgv::k_head_offsets, dim3((unsigned)hb), dim3(1024), 0, s->stream, (const unsigned long long *)(meta + off_lines),
                           (const uint32_t *)(meta + off_fields), nl, (const unsigned long long *)d_block, d_head_off);
        hipLaunchKernelGGL(hpgv::k_copy_heads, dim3((unsigned)nl), dim3(64), 0, s->stream, d_src, (const unsigned long long *)(meta + off_lines),
                           (const unsigned long long *)d_head_off, nl, d_heads);
        HIPCHK(ctx, hipGetLastError());
        unsigned long long total_heads = 0;
        HIPCHK(ctx, hipMemcpyAsync(&total_heads, d_head_off + nl, sizeof total_heads, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        if (total_heads > text_bytes) return fail(ctx, HPGV_ERR_HIP, "line heads longer than the text");
        if (total_heads) HIPCHK(ctx, hipMemcpyAsync(const_cast<char *>(text), d_heads, (size_t)total_heads, hipMemcpyDeviceToHost, s->stream));
        if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, d_head_off, ((size_t)nl + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    } else if (line_off) HIPCHK(ctx, hipMemcpyAsync(line_off, meta + off_lines, ((size_t)nl + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    if (field_off) HIPCHK(ctx, hipMemcpyAsync(field_off, meta + off_fields, (size_t)nl * 10 * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    // ---- record filters (--maf, --missing, --mendel, --inh-dom, --inh-rec: shared_options.c:44-56,101-173), from the same matrix ----
    const bool f_counts = ctx->filt_min_maf >= 0.0 || ctx->filt_max_missing >= 0.0, f_mendel = ctx->filt_max_mendel >= 0;
    const bool f_inh = ctx->filt_min_dom >= 0.0 || ctx->filt_min_rec >= 0.0;
    if (status && (f_counts || f_mendel || f_inh)) {
        const size_t n = (size_t)nl;
        std::vector<uint8_t> keep, ikeep;
        std::vector<int32_t> merr;
        if (f_inh) {
            // the assoc layout of the raw matrix, its inheritance counts and verdicts (buf[3] behind the count filters' n * 33 bytes)
            if (!ctx->assoc.set || ctx->assoc.n_samples != L.n_samples)
                return fail(ctx, HPGV_ERR_STATE, "the inheritance filters need hpgv_set_cohort over %d columns", L.n_samples);
            const size_t off8 = round_up(n * 33 + 64, 256);
            if ((rc = ensure(ctx, s, 1, n * std::max(ctx->assoc.pitch, L.pitch) + 16))) return rc;
            if ((rc = ensure(ctx, s, 3, off8 + n * 33 + 64))) return rc;
            int32_t *d_c8 = (int32_t *)((char *)s->buf[3] + off8);
            uint8_t *d_ikeep = (uint8_t *)d_c8 + n * 32;
            if ((rc = hpgv_layout_dev(ctx, HPGV_LAYOUT_ASSOC, (const uint8_t *)s->buf[7], raw_pitch, nl, (uint8_t *)s->buf[1], s->stream))) return rc;
            if ((rc = hpgv_inheritance_scan_dev(ctx, (const uint8_t *)s->buf[1], nl, d_c8, s->stream))) return rc;
            hipLaunchKernelGGL(hpgv::k_inherit_filter, dim3((nl + 255) / 256), dim3(256), 0, s->stream, (const int4 *)d_c8, nl,
                               ctx->filt_min_dom, ctx->filt_min_rec, d_ikeep);
            HIPCHK(ctx, hipGetLastError());
            ikeep.resize(n);
            HIPCHK(ctx, hipMemcpyAsync(ikeep.data(), d_ikeep, n, hipMemcpyDeviceToHost, s->stream));
        }
        if (f_counts) {
            if (!ctx->stats.set || ctx->stats.n_samples != L.n_samples)
                return fail(ctx, HPGV_ERR_STATE, "the count filters need hpgv_set_stats_cohort(%d)", L.n_samples);
            if ((rc = ensure(ctx, s, 1, n * std::max(ctx->stats.pitch, L.pitch) + 16))) return rc;
            if ((rc = ensure(ctx, s, 3, n * 33 + 64))) return rc;
            if ((rc = hpgv_layout_dev(ctx, HPGV_LAYOUT_STATS, (const uint8_t *)s->buf[7], raw_pitch, nl, (uint8_t *)s->buf[1], s->stream))) return rc;
            if ((rc = hpgv_stats_scan_dev(ctx, (const uint8_t *)s->buf[1], nl, (int32_t *)s->buf[3], s->stream))) return rc;
            uint8_t *d_keep = (uint8_t *)s->buf[3] + n * 32;
            if ((rc = hpgv_stats_filter_dev(ctx, (const int32_t *)s->buf[3], nl, ctx->filt_min_maf, -1.0, ctx->filt_max_missing, d_keep, s->stream))) return rc;
            keep.resize(n);
            HIPCHK(ctx, hipMemcpyAsync(keep.data(), d_keep, n, hipMemcpyDeviceToHost, s->stream));
        }
        if (f_mendel) {
            if (!ctx->mendel.set || ctx->mendel.n_samples != L.n_samples)
                return fail(ctx, HPGV_ERR_STATE, "the Mendelian error filter needs hpgv_set_pedigree over %d columns", L.n_samples);
            if ((rc = ensure(ctx, s, 1, n * std::max(ctx->mendel.pitch, L.pitch) + 16))) return rc;
            if ((rc = ensure(ctx, s, 4, n * sizeof(int32_t) + 64))) return rc;
            if ((rc = hpgv_layout_dev(ctx, HPGV_LAYOUT_MENDEL, (const uint8_t *)s->buf[7], raw_pitch, nl, (uint8_t *)s->buf[1], s->stream))) return rc;
            if ((rc = hpgv_mendel_scan_dev(ctx, (const uint8_t *)s->buf[1], nl, (const uint8_t *)s->buf[2], (int32_t *)s->buf[4], s->stream))) return rc;
            merr.resize(n);
            HIPCHK(ctx, hipMemcpyAsync(merr.data(), s->buf[4], n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        }
        HIPCHK(ctx, hipStreamSynchronize(s->stream));
        for (size_t i = 0; i < n; ++i) {
            const bool out = (f_counts && !keep[i]) || (f_mendel && (long)merr[i] > ctx->filt_max_mendel) || (f_inh && !ikeep[i]);
            if (out) status[i] |= HPGV_LINE_FILTERED;
        }
    }
    if (!final_layout) return HPGV_OK;                       // the caller's one-pass kernel reads the raw matrix itself
    S->d_laid = (const uint8_t *)s->buf[1]; S->which = which;
    return hpgv_layout_dev(ctx, which, (const uint8_t *)s->buf[7], raw_pitch, nl, (uint8_t *)s->buf[1], s->stream);
}

extern "C" {

int hpgv_set_text_filters(hpgv_ctx *ctx, double min_maf, double max_missing, long max_mendel_errors) {
    GROUP_ALL(ctx, hpgv_set_text_filters(m_, min_maf, max_missing, max_mendel_errors))
    if (!ctx) return HPGV_ERR_INVALID;
    if (min_maf > 0.5 || max_missing > 1.0) return fail(ctx, HPGV_ERR_INVALID, "min_maf is at most 0.5, max_missing at most 1");
    ctx->filt_min_maf = min_maf; ctx->filt_max_missing = max_missing; ctx->filt_max_mendel = max_mendel_errors;
    return HPGV_OK;
}

int hpgv_set_text_inheritance_filters(hpgv_ctx *ctx, double min_dominant, double min_recessive) {
    GROUP_ALL(ctx, hpgv_set_text_inheritance_filters(m_, min_dominant, min_recessive))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!(min_dominant <= 1.0) || !(min_recessive <= 1.0)) return fail(ctx, HPGV_ERR_INVALID, "the inheritance thresholds are at most 1");
    ctx->filt_min_dom = min_dominant < 0.0 ? -1.0 : min_dominant;
    ctx->filt_min_rec = min_recessive < 0.0 ? -1.0 : min_recessive;
    return HPGV_OK;
}

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
