// hpgv_scan_capi.hip -- C ABI of the device-resident calls (include/hpgv.h "*_dev"): layout, synthetic data, the scans and
// their statistics kernels on buffers and streams of the caller's.  The synchronous entry points of hpgv_tool_capi.hip
// run the same launchers on their slot's stream.
#include "hpgv_internal.h"
#include <type_traits>
#include "hpgv_inherit_kernels.h"

namespace {

// the wave-per-variant grid of the scans: variants_per_wave consecutive rows per wave, four waves per workgroup
unsigned scan_blocks(const hpgv_ctx *ctx, int n_variants) {
    const long waves = ((long)n_variants + ctx->vpw - 1) / ctx->vpw;
    return (unsigned)((waves + 3) / 4);
}

// what every scan checks after its cohort: the arguments, then the alignment of the rows (16 bytes) and of the output
// (out_mask).  *go = there are rows to scan
const char *const kAligned16 = "device buffers must be 16-byte aligned";
int scan_checks(hpgv_ctx *ctx, int n_variants, const void *d_gt, const void *d_out, uintptr_t out_mask, const char *align_text, bool *go) {
    *go = false;
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_out))) return fail(ctx, HPGV_ERR_INVALID, "bad scan arguments");
    if (n_variants == 0) return HPGV_OK;
    if (((uintptr_t)d_gt & 15) || ((uintptr_t)d_out & out_mask)) return fail(ctx, HPGV_ERR_INVALID, "%s", align_text);
    *go = true;
    return HPGV_OK;
}

// the scans are instantiated for non-temporal loads (shipped) and ordinary ones: f(std::true_type) or f(std::false_type)
template <typename F>
void launch_nt(const hpgv_ctx *ctx, F &&f) {
    if (ctx->nontemporal) f(std::true_type{}); else f(std::false_type{});
}

}  // namespace

extern "C" {

/* ---- layout + synth ------------------------------------------------------- */

static Layout *pick_layout(hpgv_ctx *ctx, int which) {
    switch (which) {
        case HPGV_LAYOUT_ASSOC: return &ctx->assoc;
        case HPGV_LAYOUT_TDT: return &ctx->tdt;
        case HPGV_LAYOUT_STATS: return &ctx->stats;
        case HPGV_LAYOUT_STATS_GROUPS: return &ctx->sgroups;
        case HPGV_LAYOUT_MENDEL: return &ctx->mendel;
        case HPGV_LAYOUT_EPI: return &ctx->assoc;
        default: return nullptr;
    }
}

// per-layout recoding of the stored byte (hpgv_kernels.h "Per-tool recoding")
static void recode_of(const hpgv_ctx *ctx, int which, int *mode, int *p16) {
    *mode = hpgv::RECODE_NONE; *p16 = 0;
    if (which == HPGV_LAYOUT_TDT) { *mode = hpgv::RECODE_TDT; *p16 = ctx->tdt_plan.p16; }
    else if (which == HPGV_LAYOUT_STATS || which == HPGV_LAYOUT_STATS_GROUPS) { *mode = hpgv::RECODE_STATS; }
    else if (which == HPGV_LAYOUT_MENDEL) { *mode = hpgv::RECODE_MENDEL; }
    else if (which == HPGV_LAYOUT_EPI) { *mode = hpgv::RECODE_EPI; }
}

int hpgv_layout_dev(hpgv_ctx *ctx, int which, const uint8_t *d_src, size_t src_pitch, int n_variants,
                    uint8_t *d_dst, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    Layout *L = pick_layout(ctx, which);
    if (!L) return fail(ctx, HPGV_ERR_INVALID, "unknown layout %d", which);
    if (!L->set) return fail(ctx, HPGV_ERR_STATE, "layout %d has no cohort yet", which);
    if (n_variants < 0 || (n_variants > 0 && (!d_src || !d_dst))) return fail(ctx, HPGV_ERR_INVALID, "bad layout arguments");
    if (src_pitch < (size_t)L->n_samples) return fail(ctx, HPGV_ERR_INVALID, "src_pitch %zu < n_samples %d", src_pitch, L->n_samples);
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    const int strict = (which == HPGV_LAYOUT_STATS || which == HPGV_LAYOUT_STATS_GROUPS) ? 0 : 1;
    int mode, p16;
    recode_of(ctx, which, &mode, &p16);
    // one thread per 16-byte chunk; slabs of variants keep a launch below 2^31 threads
    const long slab = std::max(1L, (1L << 31) / (L->chunks > 0 ? L->chunks : 1));
    for (long off = 0; off < n_variants; off += slab) {
        const int n = (int)std::min(slab, (long)n_variants - off);
        const long total = (long)n * L->chunks;
        hipLaunchKernelGGL(hpgv::k_layout, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           d_src + (size_t)off * src_pitch, src_pitch, n, L->pitch, L->chunks, L->d_col_of_pos(), strict, mode, p16,
                           d_dst + (size_t)off * L->pitch);
    }
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

static int synth_common(hpgv_ctx *ctx, uint64_t v0, int n_variants, size_t pitch, int chunks,
                        const int32_t *d_col, int mode, int p16, uint8_t *d_dst, hipStream_t st) {
    // generated in slabs so the threshold scratch stays small and a launch stays below 2^31 threads (one per 16-byte
    // chunk; a grid of more than 2^32 threads does not launch whole)
    const long by_threads = (1L << 31) / (chunks > 0 ? chunks : 1);
    const int slab = (int)std::max(1L, std::min((long)(1 << 20), by_threads));
    HIPCHK(ctx, ctx->d_thr.reserve((size_t)(n_variants < slab ? n_variants : slab) * 3 * sizeof(uint32_t)));
    uint32_t *d_thr = ctx->d_thr.as<uint32_t>();
    for (int off = 0; off < n_variants; off += slab) {
        const int n = (n_variants - off) < slab ? (n_variants - off) : slab;
        hipLaunchKernelGGL(hpgv::k_synth_thresholds, dim3((n + 255) / 256), dim3(256), 0, st,
                           v0 + (uint64_t)off, n, d_thr);
        const long total = (long)n * chunks;
        hipLaunchKernelGGL(hpgv::k_synth_layout, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           v0 + (uint64_t)off, n, pitch, chunks, d_col, d_thr, mode, p16,
                           d_dst + (size_t)off * pitch);
        HIPCHK(ctx, hipGetLastError());
    }
    return HPGV_OK;
}

int hpgv_synth_dev(hpgv_ctx *ctx, int which, uint64_t v0, int n_variants, uint8_t *d_dst, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    Layout *L = pick_layout(ctx, which);
    if (!L) return fail(ctx, HPGV_ERR_INVALID, "unknown layout %d", which);
    if (!L->set) return fail(ctx, HPGV_ERR_STATE, "layout %d has no cohort yet", which);
    if (n_variants < 0 || (n_variants > 0 && !d_dst)) return fail(ctx, HPGV_ERR_INVALID, "bad synth arguments");
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    int mode, p16;
    recode_of(ctx, which, &mode, &p16);
    std::lock_guard<std::mutex> lk(ctx->mu);   // shares ctx->d_thr
    return synth_common(ctx, v0, n_variants, L->pitch, L->chunks, L->d_col_of_pos(), mode, p16, d_dst, (hipStream_t)stream);
}

int hpgv_synth_raw_dev(hpgv_ctx *ctx, uint64_t v0, int n_variants, int n_samples, size_t pitch,
                       uint8_t *d_dst, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0 || n_samples < 0 || pitch % 16 || pitch < (size_t)n_samples || (n_variants > 0 && !d_dst))
        return fail(ctx, HPGV_ERR_INVALID, "bad synth_raw arguments (pitch must be a multiple of 16 >= n_samples)");
    if (n_variants == 0 || pitch == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    std::vector<int32_t> col(pitch, -1);
    for (int j = 0; j < n_samples; ++j) col[j] = j;
    int32_t *d_col = nullptr;
    HIPCHK(ctx, hipMalloc(&d_col, pitch * sizeof(int32_t)));
    hipError_t e = hipMemcpy(d_col, col.data(), pitch * sizeof(int32_t), hipMemcpyHostToDevice);
    int rc = HPGV_OK;
    if (e != hipSuccess) rc = fail(ctx, HPGV_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(e));
    if (!rc) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        rc = synth_common(ctx, v0, n_variants, pitch, (int)(pitch / 16), d_col, hpgv::RECODE_NONE, 0, d_dst, (hipStream_t)stream);
    }
    (void)hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d_col);
    return rc;
    HPGV_ABI_CATCH(ctx)
}

/* ---- assoc ------------------------------------------------------------------ */

int hpgv_assoc_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x,
                        int32_t *d_counts, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    bool go;
    if (const int rc = scan_checks(ctx, n_variants, d_gt, d_counts, 15, kAligned16, &go); rc || !go) return rc;
    DeviceGuard g(ctx->device);
    const Layout &L = ctx->assoc;
    const int vpw = (int)ctx->vpw;
    unsigned blocks = scan_blocks(ctx, n_variants);
    if (ctx->persistent) {
        const unsigned cap = (unsigned)(ctx->n_cus * ctx->blocks_per_cu);
        const unsigned need = (unsigned)(((long)n_variants + 3) / 4);
        blocks = need < cap ? need : cap;
    }
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *gt = d_gt;
    int4 *out = (int4 *)d_counts;
    const int cA = ctx->chunksA, ch = L.chunks;
    const size_t pitch = L.pitch;
#define HPGV_LAUNCH_PIPE(NT, U, W)                                                                \
    hipLaunchKernelGGL((hpgv::k_assoc_scan_pipe<NT, U, W>), dim3(blocks), dim3(256), 0, st, gt, pitch, \
                       n_variants, cA, ch, d_is_x, out, vpw)
#ifndef HPGV_ABLATION
    // the shipped form: software-pipelined, non-temporal loads, four tiles in flight, four waves per SIMD
    return launch_profiled(ctx, st, 0, [&] { HPGV_LAUNCH_PIPE(true, 4, 4); });
#else
#define HPGV_LAUNCH_ASSOC(NT, U, S)                                                              \
    hipLaunchKernelGGL((hpgv::k_assoc_scan<NT, U, S>), dim3(blocks), dim3(256), 0, st, gt, pitch, \
                       n_variants, cA, ch, d_is_x, out, vpw)
#define HPGV_DISPATCH_U(NT, S)                                                                   \
    switch (ctx->scan_unroll) {                                                                  \
        case 4: HPGV_LAUNCH_ASSOC(NT, 4, S); break;                                              \
        case 10: HPGV_LAUNCH_ASSOC(NT, 10, S); break;                                            \
        case 12: HPGV_LAUNCH_ASSOC(NT, 12, S); break;                                            \
        case 16: HPGV_LAUNCH_ASSOC(NT, 16, S); break;                                            \
        default: HPGV_LAUNCH_ASSOC(NT, 8, S); break;                                             \
    }
#define HPGV_PIPE_W(NT, U)                                                                       \
    do {                                                                                         \
        if (ctx->pipe_waves == 8) { HPGV_LAUNCH_PIPE(NT, U, 8); }                                \
        else if (ctx->pipe_waves == 6) { HPGV_LAUNCH_PIPE(NT, U, 6); }                           \
        else { HPGV_LAUNCH_PIPE(NT, U, 4); }                                                     \
    } while (0)
    if (ctx->pipeline && !ctx->persistent)
        return launch_profiled(ctx, st, 0, [&] {
            if (ctx->nontemporal) {
                if (ctx->scan_unroll <= 4) HPGV_PIPE_W(true, 4); else HPGV_PIPE_W(true, 5);
            } else {
                if (ctx->scan_unroll <= 4) HPGV_PIPE_W(false, 4); else HPGV_PIPE_W(false, 5);
            }
        });
    return launch_profiled(ctx, st, 0, [&] {
        if (ctx->nontemporal) {
            if (ctx->persistent) { HPGV_DISPATCH_U(true, true) } else { HPGV_DISPATCH_U(true, false) }
        } else {
            if (ctx->persistent) { HPGV_DISPATCH_U(false, true) } else { HPGV_DISPATCH_U(false, false) }
        }
    });
#undef HPGV_DISPATCH_U
#undef HPGV_PIPE_W
#undef HPGV_LAUNCH_ASSOC
#endif
#undef HPGV_LAUNCH_PIPE
}

int hpgv_assoc_chisq_dev(hpgv_ctx *ctx, const int32_t *d_counts, int n_variants, double *d_odds,
                         double *d_chisq, double *d_p, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0 || (n_variants > 0 && (!d_counts || !d_odds || !d_chisq || !d_p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad chisq arguments");
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    return launch_profiled(ctx, st, 1, [&] {
        hipLaunchKernelGGL(hpgv::k_assoc_chisq, dim3((n_variants + 255) / 256), dim3(256), 0, st,
                           (const int4 *)d_counts, n_variants, d_odds, d_chisq, d_p);
    });
}

int hpgv_assoc_fisher_dev(hpgv_ctx *ctx, const int32_t *d_counts, int n_variants, double *d_odds,
                          double *d_p, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0 || (n_variants > 0 && (!d_counts || !d_odds || !d_p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad fisher arguments");
    if (const int rc = logfact_check(ctx)) return rc;
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    const double cut = pow(10.0, -(double)ctx->fisher_cut_exp);
    return launch_profiled(ctx, st, 1, [&] {
        // fisher_width lanes per variant: 64 / width variants per wave, 4 waves per workgroup
        const long per_block = 4 * (64 / ctx->fisher_width);
        const unsigned blocks = (unsigned)(((long)n_variants + per_block - 1) / per_block);
#ifdef HPGV_ABLATION
        const unsigned pad = (unsigned)ctx->fisher_lds;             // experiment: unused LDS per workgroup caps the pass's waves per unit (room for a scan beside it)
        if (ctx->fisher_width == 64)
            hipLaunchKernelGGL(hpgv::k_assoc_fisher<64>, dim3(blocks), dim3(256), pad, st, (const int4 *)d_counts, n_variants, ctx->d_lf, d_odds, d_p, cut);
        else if (ctx->fisher_width == 8)
            hipLaunchKernelGGL(hpgv::k_assoc_fisher<8>, dim3(blocks), dim3(256), pad, st, (const int4 *)d_counts, n_variants, ctx->d_lf, d_odds, d_p, cut);
        else if (ctx->fisher_width == 32)
            hipLaunchKernelGGL(hpgv::k_assoc_fisher<32>, dim3(blocks), dim3(256), pad, st, (const int4 *)d_counts, n_variants, ctx->d_lf, d_odds, d_p, cut);
        else
#else
        const unsigned pad = 0u;
#endif
            hipLaunchKernelGGL(hpgv::k_assoc_fisher<16>, dim3(blocks), dim3(256), pad, st, (const int4 *)d_counts, n_variants, ctx->d_lf, d_odds, d_p, cut);
    });
}

/* ---- tdt ------------------------------------------------------------------- */

int hpgv_tdt_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x,
                      int32_t *d_tu, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->tdt.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_families has not been called");
    bool go;
    if (const int rc = scan_checks(ctx, n_variants, d_gt, d_tu, 7, "device buffers must be aligned", &go); rc || !go) return rc;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    return launch_profiled(ctx, st, 0, [&] {
        ctx->tdt_plan.launch_scan(d_gt, ctx->tdt.pitch, n_variants, d_is_x, (int2 *)d_tu,
                                  (int)ctx->vpw, ctx->nontemporal != 0, st);
    });
}

int hpgv_tdt_stats_dev(hpgv_ctx *ctx, const int32_t *d_tu, int n_variants, double *d_odds,
                       double *d_chisq, double *d_p, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0 || (n_variants > 0 && (!d_tu || !d_odds || !d_chisq || !d_p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad tdt stats arguments");
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    return launch_profiled(ctx, st, 1, [&] {
        hipLaunchKernelGGL(hpgv::k_tdt_stats, dim3((n_variants + 255) / 256), dim3(256), 0, st,
                           (const int2 *)d_tu, n_variants, d_odds, d_chisq, d_p);
    });
}

/* ---- stats ----------------------------------------------------------------- */

// one launcher for the whole row and for one group's segment of it: `chunks` 16-byte chunks from byte `off` of every row
static int stats_scan(hpgv_ctx *ctx, const Layout &L, const uint8_t *d_gt, int n_variants, uint32_t off, int chunks, size_t lds,
                      int32_t *d_counts8, hipStream_t st) {
    bool go;
    if (const int rc = scan_checks(ctx, n_variants, d_gt, d_counts8, 15, kAligned16, &go); rc || !go) return rc;
    DeviceGuard g(ctx->device);
    const int vpw = (int)ctx->vpw;
    const unsigned blocks = scan_blocks(ctx, n_variants);
    return launch_profiled(ctx, st, 0, [&] {
        launch_nt(ctx, [&](auto NT) {
            constexpr bool nt = decltype(NT)::value;
            if (ctx->pipeline)                            // bit-sliced counting, pipelined tiles (default)
                hipLaunchKernelGGL((hpgv::k_stats_scan_hs<nt>), dim3(blocks), dim3(256), nt ? lds : 0, st, d_gt, L.pitch, n_variants, off, chunks, (int4 *)d_counts8, vpw);
            else
                hipLaunchKernelGGL((hpgv::k_stats_scan<nt, kScanUnroll>), dim3(blocks), dim3(256), 0, st, d_gt, L.pitch, n_variants, off, chunks, (int4 *)d_counts8, vpw);
        });
    });
}

int hpgv_stats_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_counts8, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    const Layout &L = ctx->stats;
    // rows of 6.5 KB or more stream best with three workgroups (12 waves) per compute unit -- 48 KB of unused LDS per workgroup:
    // 1M x 10k: 1.59 -> 1.53 ms, 7 000 samples +4 %, 50k / 100k samples +1 - 2 %; shorter rows need every wave (5 000 samples: -12 %
    // with the cap).  Option scan_lds > 0 sets the bytes.
    const size_t scan_lds = ctx->scan_lds > 0 ? (size_t)ctx->scan_lds : (L.pitch >= 6656 ? (size_t)49152 : (size_t)0);
    return stats_scan(ctx, L, d_gt, n_variants, 0u, L.chunks, scan_lds, d_counts8, (hipStream_t)stream);
}

int hpgv_stats_scan_group_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int group, int32_t *d_counts8, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->sgroups.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_groups has not been called");
    if (group < 0 || (size_t)group >= ctx->sg_off.size()) return fail(ctx, HPGV_ERR_INVALID, "group %d out of range", group);
    const int chunks = (int)(round_up((size_t)ctx->sg_size[(size_t)group], 16) / 16);
    return stats_scan(ctx, ctx->sgroups, d_gt, n_variants, ctx->sg_off[(size_t)group], chunks, 0, d_counts8, (hipStream_t)stream);
}

int hpgv_stats_hwe_dev(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants, double *d_chi2,
                       double *d_p, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_variants < 0 || (n_variants > 0 && (!d_counts8 || !d_chi2 || !d_p)))
        return fail(ctx, HPGV_ERR_INVALID, "bad hwe arguments");
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    hipStream_t st = (hipStream_t)stream;
    return launch_profiled(ctx, st, 1, [&] {
        hipLaunchKernelGGL(hpgv::k_stats_hwe, dim3((n_variants + 255) / 256), dim3(256), 0, st,
                           (const int4 *)d_counts8, n_variants, d_chi2, d_p);
    });
}

int hpgv_mendel_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x, int32_t *d_errors, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->mendel.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_pedigree has not been called");
    bool go;
    if (const int rc = scan_checks(ctx, n_variants, d_gt, d_errors, 0, kAligned16, &go); rc || !go) return rc;
    DeviceGuard g(ctx->device);
    const int vpw = (int)ctx->vpw;
    const unsigned blocks = scan_blocks(ctx, n_variants);
    hipStream_t st = (hipStream_t)stream;
    return launch_profiled(ctx, st, 0, [&] {
        launch_nt(ctx, [&](auto NT) {
            hipLaunchKernelGGL((hpgv::k_mendel_scan<decltype(NT)::value, 4>), dim3(blocks), dim3(256), 0, st, d_gt, ctx->mendel.pitch, n_variants,
                               ctx->mendel_pchunks, ctx->mendel_luts, ctx->d_mendel_male, d_is_x, d_errors, vpw);
        });
    });
}

int hpgv_mendel_children_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, const uint8_t *d_is_x,
                             int32_t *d_child_errors, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->mendel.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_pedigree has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_child_errors))) return fail(ctx, HPGV_ERR_INVALID, "bad scan arguments");
    if (n_variants == 0 || ctx->mendel_trios == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    const unsigned tiles = (unsigned)((ctx->mendel_pchunks + 63) / 64);
    dim3 grid((tiles + 3) / 4, (unsigned)((n_variants + hpgv::SAMPLE_STATS_ROWS - 1) / hpgv::SAMPLE_STATS_ROWS));
    if (grid.y > 65535u) return fail(ctx, HPGV_ERR_UNSUPPORTED, "more than %d variants per call", 65535 * hpgv::SAMPLE_STATS_ROWS);
    hipLaunchKernelGGL(hpgv::k_mendel_children, grid, dim3(256), 0, (hipStream_t)stream, d_gt, ctx->mendel.pitch, n_variants,
                       ctx->mendel_pchunks, ctx->mendel_trios, ctx->mendel_luts, ctx->d_mendel_male, d_is_x, d_child_errors);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_stats_filter_dev(hpgv_ctx *ctx, const int32_t *d_counts8, int n_variants, double min_maf, double max_maf,
                          double max_missing, uint8_t *d_keep, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!d_counts8 || !d_keep))) return fail(ctx, HPGV_ERR_INVALID, "bad filter arguments");
    if (n_variants == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    hipLaunchKernelGGL(hpgv::k_stats_filter, dim3((n_variants + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const int4 *)d_counts8, n_variants, ctx->stats.n_samples, min_maf, max_maf, max_missing, d_keep);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_inheritance_scan_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_counts8, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    bool go;
    if (const int rc = scan_checks(ctx, n_variants, d_gt, d_counts8, 15, kAligned16, &go); rc || !go) return rc;
    DeviceGuard g(ctx->device);
    const Layout &L = ctx->assoc;
    const int vpw = (int)ctx->vpw;
    const unsigned blocks = scan_blocks(ctx, n_variants);
    hipStream_t st = (hipStream_t)stream;
    return launch_profiled(ctx, st, 0, [&] {
        launch_nt(ctx, [&](auto NT) {
            hipLaunchKernelGGL((hpgv::k_inherit_scan<decltype(NT)::value, 4>), dim3(blocks), dim3(256), 0, st, d_gt, L.pitch, n_variants, ctx->chunksA,
                               L.chunks, (int4 *)d_counts8, vpw);
        });
    });
}

int hpgv_sample_missing_dev(hpgv_ctx *ctx, const uint8_t *d_gt, int n_variants, int32_t *d_missing, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (n_variants < 0 || (n_variants > 0 && (!d_gt || !d_missing))) return fail(ctx, HPGV_ERR_INVALID, "bad sample stats arguments");
    if (n_variants == 0 || ctx->stats.n_samples == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    const Layout &L = ctx->stats;
    const unsigned tiles = (unsigned)((L.chunks + 63) / 64);
    dim3 grid((tiles + 3) / 4, (unsigned)((n_variants + hpgv::SAMPLE_STATS_ROWS - 1) / hpgv::SAMPLE_STATS_ROWS));
    if (grid.y > 65535u) return fail(ctx, HPGV_ERR_UNSUPPORTED, "more than %d variants per sample-stats call", 65535 * hpgv::SAMPLE_STATS_ROWS);
    hipLaunchKernelGGL(hpgv::k_sample_missing, grid, dim3(256), 0, (hipStream_t)stream, d_gt, L.pitch, n_variants,
                       L.chunks, L.n_samples, d_missing);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_genotype_table_dev(hpgv_ctx *ctx, const uint8_t *d_raw, size_t src_pitch, int n_samples,
                            const int32_t *d_variant_idx, int n_idx, int32_t *d_table, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_idx < 0 || n_samples < 0 || (n_idx > 0 && (!d_raw || !d_table)) || src_pitch < (size_t)n_samples)
        return fail(ctx, HPGV_ERR_INVALID, "bad genotype table arguments");
    if (n_idx == 0) return HPGV_OK;
    DeviceGuard g(ctx->device);
    hipLaunchKernelGGL(hpgv::k_genotype_table, dim3((unsigned)n_idx), dim3(256), 0, (hipStream_t)stream, d_raw, src_pitch,
                       n_samples, d_variant_idx, n_idx, d_table);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

int hpgv_last_kernel_ms(hpgv_ctx *ctx, float *scan_ms, float *stats_ms) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    if (scan_ms) {
        *scan_ms = -1.f;
        if (ctx->have_scan_ev) {
            HIPCHK(ctx, hipEventSynchronize(ctx->ev[1]));
            HIPCHK(ctx, hipEventElapsedTime(scan_ms, ctx->ev[0], ctx->ev[1]));
        }
    }
    if (stats_ms) {
        *stats_ms = -1.f;
        if (ctx->have_stats_ev) {
            HIPCHK(ctx, hipEventSynchronize(ctx->ev[3]));
            HIPCHK(ctx, hipEventElapsedTime(stats_ms, ctx->ev[2], ctx->ev[3]));
        }
    }
    return HPGV_OK;
}

int hpgv_read_probe(hpgv_ctx *ctx, const uint8_t *d_buf, size_t bytes, int iters, float *ms) {
    ctx = first_member(ctx);
    if (!ctx || !d_buf || !ms || iters <= 0 || ((uintptr_t)d_buf & 15)) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    const size_t n16 = bytes / 16;
    hipEvent_t a, b;
    HIPCHK(ctx, hipEventCreate(&a));
    HIPCHK(ctx, hipEventCreate(&b));
    const unsigned blocks = (unsigned)(ctx->n_cus * 4);      // 4 blocks x 4 waves per CU: the pipelined scan's occupancy
    auto go = [&] {
        launch_nt(ctx, [&](auto NT) {
            hipLaunchKernelGGL((hpgv::k_read_probe<decltype(NT)::value>), dim3(blocks), dim3(256), 0, nullptr, (const uint4 *)d_buf, n16, ctx->d_sink);
        });
    };
    go();
    HIPCHK(ctx, hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) go();
    HIPCHK(ctx, hipEventRecord(b, nullptr));
    HIPCHK(ctx, hipEventSynchronize(b));
    float t = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&t, a, b));
    *ms = t / iters;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return HPGV_OK;
}

}  // extern "C"
