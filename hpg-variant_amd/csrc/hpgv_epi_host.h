// hpgv_epi_host.h -- host side of the epistasis rankings, shared by hpgv_epi_capi.hip (pairs, triples), hpgv_epi_generic_capi.hip
// (any order) and hpgv_group_capi.hip (the gather over a group's devices): the one model record with its order, the checks and
// fold constants every entry point repeats, and the ONE ranking loop -- launch, read the candidate lists back, repeat smaller
// after an overflow, merge into the per-fold top lists, raise the thresholds.
#pragma once
#include "hpgv_internal.h"
#include <tuple>

// a ranked model of any order, and the record of the group's gather (used = 0: an empty slot)
struct EpiModel {
    double accuracy;
    int32_t c[5];                      // its SNPs in ascending order, -1 past the order
    int32_t used;
    uint32_t risky[hpgv::EPI_MASK_WORDS];      // bit c = cell c is high risk; orders 2 and 3 fill word 0
};
static_assert(sizeof(EpiModel) == 64, "one record of the gathered top lists");

// add_to_model_ranking, model.c:478-517: higher accuracy, then the smaller combination -- of model records and of the pair and
// triple kernels' own candidate records, which the ranking loop merges as they come (epi_snps: the combination as a sort key)
inline std::tuple<int32_t, int32_t, int32_t, int32_t, int32_t> epi_snps(const EpiModel &m) { return {m.c[0], m.c[1], m.c[2], m.c[3], m.c[4]}; }
inline std::tuple<int32_t, int32_t> epi_snps(const hpgv::EpiCand &c) { return {c.i, c.j}; }
inline std::tuple<int32_t, int32_t, int32_t> epi_snps(const hpgv::EpiCand3 &c) { return {c.i, c.j, c.k}; }
template <class R>
bool epi_better(const R &a, const R &b) { return a.accuracy != b.accuracy ? a.accuracy > b.accuracy : epi_snps(a) < epi_snps(b); }

inline const EpiModel &epi_model(const EpiModel &m) { return m; }
inline EpiModel epi_model(const hpgv::EpiCand &c) { return EpiModel{c.accuracy, {c.i, c.j, -1, -1, -1}, 1, {c.risky}}; }
inline EpiModel epi_model(const hpgv::EpiCand3 &c) { return EpiModel{c.accuracy, {c.i, c.j, c.k, -1, -1}, 1, {c.risky}}; }

// per-fold rankings of the combinations whose first SNP lies in [i_begin, i_end): out[f * N + e], `used` up to the list's length.
// ctx is a device's own context; have_outputs: the caller's output pointers are all there ("bad ranking arguments" otherwise,
// in the order the public entry points have always checked).  Defined in hpgv_epi_capi.hip and hpgv_epi_generic_capi.hip.
int hpgv_epi_pairs_models(hpgv_ctx *ctx, int i_begin, int i_end, int subset, int N, bool have_outputs, std::vector<EpiModel> &out, float *scan_ms);
int hpgv_epi_triples_models(hpgv_ctx *ctx, int i_begin, int i_end, int subset, int N, bool have_outputs, std::vector<EpiModel> &out, float *scan_ms);
int hpgv_epi_order_models(hpgv_ctx *ctx, int order, int i_begin, int i_end, int subset, int N, bool have_outputs, std::vector<EpiModel> &out, float *scan_ms);

namespace {

struct EventPair {                                                   // the two timing events of a ranking call
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
struct DevFree { void *p = nullptr; ~DevFree() { if (p) (void)hipFree(p); } };

inline int epi_check_folds(const hpgv_ctx *ctx) {
    if (!ctx->epi.have_folds) return fail(ctx, HPGV_ERR_STATE, "no folds: hpgv_epi_set_dataset has not been called, or a class of 65536 samples or more waits for hpgv_epi_set_folds");
    return HPGV_OK;
}
// the shape is past the packed kernels (16-bit counts per group and per class, EPI_MAX_FOLDS folds): its listed-combination
// launches are k_epi_combs_wide, and its triple (and, for a wide-only layout, pair) rankings go through the any-order ranking.
// A wide-only layout exists only because option "epi_wide" allowed it; it stays wide whatever the option says later.
inline bool epi_needs_wide(const hpgv_ctx *ctx) {
    const EpiState &E = ctx->epi;
    return E.wide_only || (ctx->epi_wide >= 1 && (E.nA > 65535 || E.nU > 65535));
}
inline int epi_refuse_dense_wide(const hpgv_ctx *ctx, const char *what) {
    return fail(ctx, HPGV_ERR_UNSUPPORTED, "the dense %s scan does not take a wide layout (more than %d folds, or 65536 samples or more of one class in one fold): evaluate listed combinations with hpgv_epi_eval_combs",
                what, hpgv::EPI_MAX_FOLDS);
}
inline int epi_check_subset(const hpgv_ctx *ctx, int subset) {
    if (subset != HPGV_EPI_TESTING && subset != HPGV_EPI_TRAINING) return fail(ctx, HPGV_ERR_INVALID, "subset must be HPGV_EPI_TESTING or HPGV_EPI_TRAINING");
    return HPGV_OK;
}
inline int epi_check(const hpgv_ctx *ctx, int subset) {
    if (int rc = epi_check_folds(ctx)) return rc;
    return epi_check_subset(ctx, subset);
}

// per fold: testing sizes and the reciprocals of the evaluated part's sizes (RN(1 / y): IEEE double division on the host), for
// the scan kernels' evaluation
inline int epi_upload_folds(hpgv_ctx *ctx, bool training, hipStream_t st) {
    EpiState &E = ctx->epi;
    hpgv::EpiFold folds[hpgv::EPI_WIDE_MAX_FOLDS];
    for (int f = 0; f < E.fold_cap; ++f) {                           // (slots past num_folds: test_a = -1, unused)
        folds[f].test_a = E.group_size[(size_t)2 * f]; folds[f].test_u = E.group_size[(size_t)2 * f + 1];
        const int sa = training ? E.nA - folds[f].test_a : folds[f].test_a, su = training ? E.nU - folds[f].test_u : folds[f].test_u;
        folds[f].inv_a = 1.0 / (double)sa; folds[f].inv_u = 1.0 / (double)su;
    }
    HIPCHK(ctx, hipMemcpyAsync(E.d_folds, folds, (size_t)E.fold_cap * sizeof(hpgv::EpiFold), hipMemcpyHostToDevice, st));
    return HPGV_OK;
}

// The ranking loop of every order.  `o` is the order's launch policy:
//   Cand                the candidate record its kernel lists
//   setup()             makes d_cand: a list of `cap` records per fold
//   more()              something is left to scan
//   launch()            cuts the next launch and queues it on the null stream (what it queues is what scan_ms times)
//   shrink()            a list overflowed: makes that launch smaller, or refuses
//   advance(worst)      the launch is merged (its longest list held `worst` models): moves on, grows
//   keep(cand)          the candidate as the top lists hold it: as it is, or -- where it names its combination by a position in
//                       the launch's list -- as a model record
// The order of the launches does not show in the ranking: ties go by the combination.
template <class Order>
int epi_rank_loop(hpgv_ctx *ctx, Order &o, int N, std::vector<EpiModel> &out, float *scan_ms) {
    using Cand = typename Order::Cand;
    EpiState &E = ctx->epi;
    E.rank_info = hpgv_epi_rank_info{};
    if (int rc = o.setup()) return rc;
    const int nf = E.num_folds, slots = E.fold_cap;                  // the kernels instantiated per fold count read `slots` thresholds
    if (E.rank_fold_cap < slots) {                                     // (the layout before this one had fewer folds)
        if (E.d_cand_count) (void)hipFree(E.d_cand_count);
        if (E.d_thr) (void)hipFree(E.d_thr);
        E.d_cand_count = nullptr; E.d_thr = nullptr; E.rank_fold_cap = 0;
        HIPCHK(ctx, hipMalloc(&E.d_cand_count, (size_t)slots * sizeof(unsigned)));
        HIPCHK(ctx, hipMalloc(&E.d_thr, (size_t)slots * sizeof(double)));
        E.rank_fold_cap = slots;
    }
    using Top = std::decay_t<decltype(o.keep(std::declval<const Cand &>()))>;
    std::vector<std::vector<Top>> top((size_t)nf);
    std::vector<double> thr((size_t)slots, -HUGE_VAL);
    std::vector<unsigned> count((size_t)slots);
    std::vector<Cand> buf;
    EventPair ev;                                                    // destroyed on every return path
    float total_ms = 0.f;
    if (scan_ms) { HIPCHK(ctx, hipEventCreate(&ev.a)); HIPCHK(ctx, hipEventCreate(&ev.b)); }
    while (o.more()) {
        HIPCHK(ctx, hipMemsetAsync(E.d_cand_count, 0, (size_t)slots * sizeof(unsigned), nullptr));
        HIPCHK(ctx, hipMemcpyAsync(E.d_thr, thr.data(), (size_t)slots * sizeof(double), hipMemcpyHostToDevice, nullptr));
        if (scan_ms) HIPCHK(ctx, hipEventRecord(ev.a, nullptr));
        if (int rc = o.launch()) return rc;
        if (scan_ms) HIPCHK(ctx, hipEventRecord(ev.b, nullptr));
        HIPCHK(ctx, hipMemcpy(count.data(), E.d_cand_count, (size_t)slots * sizeof(unsigned), hipMemcpyDeviceToHost));
        if (scan_ms) { float ms = 0.f; HIPCHK(ctx, hipEventElapsedTime(&ms, ev.a, ev.b)); total_ms += ms; }
        unsigned worst = 0;
        for (int f = 0; f < nf; ++f) worst = std::max(worst, count[(size_t)f]);
        if (worst > o.cap) {                                         // some list overflowed: the same part again, in smaller pieces
            ++E.rank_info.relaunches;
            if (int rc = o.shrink()) return rc;
            continue;
        }
        for (int f = 0; f < nf; ++f) {
            const unsigned n = count[(size_t)f];
            if (!n) continue;
            buf.resize(n);
            HIPCHK(ctx, hipMemcpy(buf.data(), o.d_cand + (size_t)f * o.cap, (size_t)n * sizeof(Cand), hipMemcpyDeviceToHost));
            auto &t = top[(size_t)f];
            if constexpr (std::is_same<Top, Cand>::value) t.insert(t.end(), buf.begin(), buf.end());
            else for (const Cand &c : buf) t.push_back(o.keep(c));
            if ((int)t.size() > N) { std::partial_sort(t.begin(), t.begin() + N, t.end(), epi_better<Top>); t.resize((size_t)N); }
            else std::sort(t.begin(), t.end(), epi_better<Top>);
            if ((int)t.size() >= N && t.back().accuracy > thr[(size_t)f]) thr[(size_t)f] = t.back().accuracy;
        }
        if (int rc = o.advance(worst)) return rc;
    }
    out.assign((size_t)nf * (size_t)N, EpiModel{});
    for (int f = 0; f < nf; ++f)
        std::transform(top[(size_t)f].begin(), top[(size_t)f].end(), out.begin() + (size_t)f * (size_t)N, [](const Top &t) { return epi_model(t); });
    if (scan_ms) *scan_ms = total_ms;
    return HPGV_OK;
}

// the records in a public output layout: SNP s of model o at comb[s][o * comb_stride], `mask_words` mask words per model
inline void epi_scatter(const std::vector<EpiModel> &m, int N, int order, int32_t *const *comb, size_t comb_stride, double *accuracy,
                        uint32_t *risky_mask, int mask_words, int32_t *n_ranked) {
    for (size_t f = 0; f < m.size() / (size_t)N; ++f) {
        size_t o = f * (size_t)N;
        for (; o < (f + 1) * (size_t)N && m[o].used; ++o) {
            for (int s = 0; s < order; ++s) comb[s][o * comb_stride] = m[o].c[s];
            accuracy[o] = m[o].accuracy;
            std::copy(m[o].risky, m[o].risky + mask_words, risky_mask + o * (size_t)mask_words);
        }
        n_ranked[f] = (int32_t)(o - f * (size_t)N);
    }
}

}  // namespace
