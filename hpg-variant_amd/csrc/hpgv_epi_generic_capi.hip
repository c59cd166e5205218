// hpgv_epi_generic_capi.hip -- C ABI of the MDR model for combinations of any order the reference's `--order` accepts
// (main_epistasis.c:128,142; model.c:76-206; epistasis.c:14-95), here 2 <= order <= 5: listed combinations evaluated
// (hpgv_epi_eval_combs), every combination of the dataset ranked per fold (hpgv_epi_rank_order[_rows]), and the in-fold
// counts behind hpgv_epi_counts / hpgv_epi_counts_all_folds for the orders the pair / triple kernels do not take.
// Kernel: hpgv_epi_generic_kernels.h (one lane per cell).  Its own translation unit: the pair and triple scans of
// hpgv_epi_capi.hip compile for minutes.
#include "hpgv_epi_host.h"
#include "hpgv_epi_generic_kernels.h"
#include "hpgv_epi_wide_kernels.h"

namespace {

int generic_check(hpgv_ctx *ctx, int order) {
    EpiState &E = ctx->epi;
    if (order < 2 || order > 5) return fail(ctx, HPGV_ERR_UNSUPPORTED, "combinations of %d SNPs are not supported (2 to 5)", order);
    if ((E.nA > 65535 || E.nU > 65535) && !epi_needs_wide(ctx)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "the listed-combination kernel keeps 16-bit class totals: at most 65535 samples per class");
    return HPGV_OK;
}

// d_combs: n_combs x order SNP indices on the device.  counts only: d_counts given, everything else NULL.
int launch_combs(hpgv_ctx *ctx, int order, bool training, const int32_t *d_combs, int n_combs, int32_t *d_counts, bool evaluate,
                 double *d_acc, uint32_t *d_mask, const double *d_thr, hpgv::EpiCandN *d_cand, unsigned *d_cand_count, unsigned cap) {
    EpiState &E = ctx->epi;
    if (n_combs <= 0) return HPGV_OK;
    const hpgv::EpiFold *folds = evaluate ? E.d_folds : nullptr;
    // the wide kernel (hpgv_epi_wide_kernels.h) where the packed one's 16-bit halves or fold arrays do not hold the shape, and
    // everywhere with option "epi_wide" = 2
    const bool wide = epi_needs_wide(ctx) || ctx->epi_wide == 2;
    if (d_cand) {                                                    // a ranking call's launch (hpgv_epi_last_rank_info)
        E.rank_info.kernel = wide ? HPGV_EPI_KERNEL_COMBS_WIDE : HPGV_EPI_KERNEL_COMBS;
        ++E.rank_info.launches;
    }
#define HPGV_COMBS_WIDE(ORD, TR)                                                                                                  \
    hipLaunchKernelGGL((hpgv::k_epi_combs_wide<ORD, TR>), dim3((unsigned)((n_combs + (256 / hpgv::EpiCells<ORD>::value) - 1) / (256 / hpgv::EpiCells<ORD>::value))), \
                       dim3(256), hpgv::epi_wide_lds_bytes<ORD>(E.num_folds), nullptr, E.d_planes, E.W, d_combs, n_combs, E.d_group_w0, E.num_folds, folds, E.nA, E.nU, \
                       d_counts, d_acc, d_mask, d_thr, d_cand, d_cand_count, cap)
#define HPGV_COMBS_WIDE_T(ORD) do { if (training) HPGV_COMBS_WIDE(ORD, true); else HPGV_COMBS_WIDE(ORD, false); } while (0)
    if (wide) {
        switch (order) {
            case 2: HPGV_COMBS_WIDE_T(2); break;
            case 3: HPGV_COMBS_WIDE_T(3); break;
            case 4: HPGV_COMBS_WIDE_T(4); break;
            default: HPGV_COMBS_WIDE_T(5); break;
        }
        HIPCHK(ctx, hipGetLastError());
        return HPGV_OK;
    }
#undef HPGV_COMBS_WIDE_T
#undef HPGV_COMBS_WIDE
#define HPGV_COMBS(ORD, TR)                                                                                                       \
    hipLaunchKernelGGL((hpgv::k_epi_combs<ORD, TR>), dim3((unsigned)((n_combs + (256 / hpgv::EpiCells<ORD>::value) - 1) / (256 / hpgv::EpiCells<ORD>::value))), \
                       dim3(256), 0, nullptr, E.d_planes, E.W, d_combs, n_combs, E.d_group_w0, E.num_folds, folds, E.nA, E.nU, d_counts, \
                       d_acc, d_mask, d_thr, d_cand, d_cand_count, cap)
#define HPGV_COMBS_T(ORD) do { if (training) HPGV_COMBS(ORD, true); else HPGV_COMBS(ORD, false); } while (0)
    switch (order) {
        case 2: HPGV_COMBS_T(2); break;
        case 3: HPGV_COMBS_T(3); break;
        case 4: HPGV_COMBS_T(4); break;
        default: HPGV_COMBS_T(5); break;
    }
#undef HPGV_COMBS_T
#undef HPGV_COMBS
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

// the next combination in lexicographic order; false after the last
bool next_comb(int32_t *c, int order, int V) {
    int s = order - 1;
    while (s >= 0 && c[s] == V - order + s) --s;
    if (s < 0) return false;
    ++c[s];
    for (int k = s + 1; k < order; ++k) c[k] = c[k - 1] + 1;
    return true;
}

// Any order.  Every combination is listed, in lexicographic order, `limit` of them per launch = at most the capacity of a fold's
// candidate list, so no list overflows.  The first launch has no thresholds and lists every combination it evaluates: a short
// one, so that the long ones that follow have bounds to filter with (131 072 models x folds x 64 bytes over the bus and a sort
// otherwise).
struct EpiListOrder {
    using Cand = hpgv::EpiCandN;
    static constexpr unsigned CHUNK = 1u << 17;
    hpgv_ctx *ctx; EpiState &E; const int order, i_end; const bool training;
    Cand *d_cand = nullptr; unsigned cap = CHUNK;
    DevFree dc, dcand;
    std::vector<int32_t> list;                                       // the launch's combinations
    int32_t cur[5];                                                  // the next one
    bool any;
    unsigned n = 0, limit;
    EpiListOrder(hpgv_ctx *c, int order_, int i_begin, int i_end_, int subset, int N)
        : ctx(c), E(c->epi), order(order_), i_end(i_end_), training(subset == HPGV_EPI_TRAINING),
          any(!(E.V < order || i_begin >= i_end || i_begin > E.V - order)), limit(std::min<unsigned>(CHUNK, (unsigned)std::max(4096, 4 * N))) {
        for (int s = 0; s < 5; ++s) cur[s] = i_begin + s;
    }
    int setup() {
        if (!any) return HPGV_OK;
        HIPCHK(ctx, hipMalloc(&dc.p, (size_t)CHUNK * (size_t)order * sizeof(int32_t)));
        HIPCHK(ctx, hipMalloc(&dcand.p, (size_t)E.num_folds * CHUNK * sizeof(Cand)));
        d_cand = (Cand *)dcand.p;
        list.resize((size_t)CHUNK * (size_t)order);
        if (int rc = epi_upload_folds(ctx, training, nullptr)) return rc;
        return stage();
    }
    int stage() {                                                    // the next launch's list, on the device before its launch is timed
        for (n = 0; any && n < limit; ++n) {
            std::copy(cur, cur + order, &list[(size_t)n * (size_t)order]);
            any = next_comb(cur, order, E.V) && cur[0] < i_end;
        }
        if (n) HIPCHK(ctx, hipMemcpyAsync(dc.p, list.data(), (size_t)n * (size_t)order * sizeof(int32_t), hipMemcpyHostToDevice, nullptr));
        return HPGV_OK;
    }
    bool more() const { return n > 0; }
    int launch() { return launch_combs(ctx, order, training, (const int32_t *)dc.p, (int)n, nullptr, true, nullptr, nullptr, E.d_thr, d_cand, E.d_cand_count, CHUNK); }
    int shrink() { return fail(ctx, HPGV_ERR_UNSUPPORTED, "a launch of %u listed combinations overflowed a candidate list", n); }
    int advance(unsigned) { limit = CHUNK; return stage(); }
    EpiModel keep(const Cand &e) const {
        EpiModel m{e.accuracy, {-1, -1, -1, -1, -1}, 1, {}};
        std::copy(&list[(size_t)e.index * (size_t)order], &list[(size_t)e.index * (size_t)order] + order, m.c);
        std::copy(e.risky, e.risky + hpgv::EPI_MASK_WORDS, m.risky);
        return m;
    }
};

}  // namespace

// in-fold counts of listed combinations, device to device: d_out[(comb * n_groups + g) * 3^order + cell] (epi_infold_counts of
// hpgv_epi_capi.hip for the orders its own kernel does not take).  The caller holds epi_mu.
int hpgv_epi_generic_counts(hpgv_ctx *ctx, int order, const int32_t *d_combs, int n_combs, int32_t *d_out) {
    int rc = generic_check(ctx, order);
    if (rc) return rc;
    return launch_combs(ctx, order, false, d_combs, n_combs, d_out, false, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
}

extern "C" {

int hpgv_epi_eval_combs(hpgv_ctx *ctx, int order, const int32_t *combs, int n_combs, int subset, double *accuracy, uint32_t *risky_mask) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    std::lock_guard<std::mutex> lk(ctx->epi_mu);
    int rc = epi_check_folds(ctx);
    if (!rc) rc = generic_check(ctx, order);
    if (!rc) rc = epi_check_subset(ctx, subset);
    if (rc) return rc;
    EpiState &E = ctx->epi;
    if (n_combs < 0 || (n_combs > 0 && (!combs || !accuracy))) return fail(ctx, HPGV_ERR_INVALID, "bad combination list");
    for (long k = 0; k < (long)n_combs * order; ++k)
        if (combs[k] < 0 || combs[k] >= E.V) return fail(ctx, HPGV_ERR_INVALID, "SNP index %d outside the dataset", combs[k]);
    if (n_combs == 0) return HPGV_OK;
    const size_t nf = (size_t)E.num_folds, n = (size_t)n_combs;
    DevFree dc, da, dm;
    HIPCHK(ctx, hipMalloc(&dc.p, n * (size_t)order * sizeof(int32_t)));
    HIPCHK(ctx, hipMalloc(&da.p, n * nf * sizeof(double)));
    if (risky_mask) HIPCHK(ctx, hipMalloc(&dm.p, n * nf * hpgv::EPI_MASK_WORDS * sizeof(uint32_t)));
    HIPCHK(ctx, hipMemcpy(dc.p, combs, n * (size_t)order * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemset(da.p, 0xFF, n * nf * sizeof(double)));      // (a fold without samples keeps NaN)
    if (dm.p) HIPCHK(ctx, hipMemset(dm.p, 0, n * nf * hpgv::EPI_MASK_WORDS * sizeof(uint32_t)));
    rc = epi_upload_folds(ctx, subset == HPGV_EPI_TRAINING, nullptr);
    if (rc) return rc;
    rc = launch_combs(ctx, order, subset == HPGV_EPI_TRAINING, (const int32_t *)dc.p, n_combs, nullptr, true, (double *)da.p, (uint32_t *)dm.p,
                      nullptr, nullptr, nullptr, 0);
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpy(accuracy, da.p, n * nf * sizeof(double), hipMemcpyDeviceToHost));
    if (risky_mask) HIPCHK(ctx, hipMemcpy(risky_mask, dm.p, n * nf * hpgv::EPI_MASK_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_epi_rank_order_rows(hpgv_ctx *ctx, int order, int i_begin, int i_end, int subset, int max_ranking_size, int32_t *combs_out,
                             double *accuracy, uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    std::vector<EpiModel> m;
    if (int rc = hpgv_epi_order_models(ctx, order, i_begin, i_end, subset, max_ranking_size, combs_out && accuracy && risky_mask && n_ranked, m, scan_ms)) return rc;
    int32_t *const comb[5] = {combs_out, combs_out + 1, combs_out + 2, combs_out + 3, combs_out + 4};
    epi_scatter(m, max_ranking_size, order, comb, (size_t)order, accuracy, risky_mask, hpgv::EPI_MASK_WORDS, n_ranked);
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

int hpgv_epi_rank_order(hpgv_ctx *ctx, int order, int subset, int max_ranking_size, int32_t *combs_out, double *accuracy,
                        uint32_t *risky_mask, int32_t *n_ranked, float *scan_ms) {
    const hpgv_ctx *c = first_member(ctx);
    return hpgv_epi_rank_order_rows(ctx, order, 0, c ? c->epi.V : 0, subset, max_ranking_size, combs_out, accuracy, risky_mask, n_ranked, scan_ms);
}

}  // extern "C"

int hpgv_epi_order_models(hpgv_ctx *ctx, int order, int i_begin, int i_end, int subset, int N, bool have_outputs, std::vector<EpiModel> &out, float *scan_ms) {
    DeviceGuard g(ctx->device);
    std::lock_guard<std::mutex> lk(ctx->epi_mu);
    int rc = epi_check_folds(ctx);
    if (!rc) rc = generic_check(ctx, order);
    if (!rc) rc = epi_check_subset(ctx, subset);
    if (rc) return rc;
    if (i_begin < 0 || i_end < i_begin || i_end > ctx->epi.V) return fail(ctx, HPGV_ERR_INVALID, "first SNPs [%d, %d) outside the dataset", i_begin, i_end);
    if (N < 1 || N > 65536 || !have_outputs) return fail(ctx, HPGV_ERR_INVALID, "bad ranking arguments");
    EpiListOrder o(ctx, order, i_begin, i_end, subset, N);
    return epi_rank_loop(ctx, o, N, out, scan_ms);
}
