// hpgv_capi.hip -- C ABI (include/hpgv.h) over the gfx950 kernels: contexts and their options, the cohort / pedigree /
// group setters and their layouts, device and host memory, streams, copies, text aliases.  The launchers are in
// hpgv_scan_capi.hip (device-resident *_dev calls), hpgv_text_capi.hip (tokenizer, front half of the text entry points),
// hpgv_tool_capi.hip (per-batch and text entry points) and hpgv_lines_capi.hip (partition and split of lines).
//
// There is no CPU path in this library: every entry point that computes
// launches HIP kernels, and hpgv_create() fails without a device.
#include "hpgv_internal.h"
#include <cstdlib>

extern "C" {

const char *hpgv_version(void) { return "hpgv-mi355x 0.1 (gfx950)"; }

int hpgv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

const char *hpgv_last_error(const hpgv_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// The environment is read HERE, once per context, and nowhere else in the library (include/hpgv.h "Environment").
static void read_environment(hpgv_ctx *ctx) {
    auto num = [](const char *name, long lo, long hi, long *out) { const char *e = getenv(name); if (e && *e) { long v = atol(e); *out = v < lo ? lo : v > hi ? hi : v; } };
    num("HPGV_BATCH_COPY", 0, 1, &ctx->batch_copy);
    num("HPGV_BATCH_FUSED", 0, 1, &ctx->batch_fused);
    num("HPGV_STATS_ALL2", 0, 1, &ctx->stats_all2);
    num("HPGV_ASSOC_ROWS", 0, 1, &ctx->assoc_rows);
    num("HPGV_PINNED_NONCOHERENT", 0, 1, &ctx->pinned_noncoherent);
    num("HPGV_VMM_TRACE", 0, 1, &ctx->vmm_trace);
    num("HPGV_DECODE_TILES", 0, 1, &ctx->decode_tiles);
#ifdef HPGV_ABLATION
    num("HPGV_INFLATE_WAVE", 0, 4, &ctx->inflate_wave);
    num("HPGV_TOKENIZER_TILES", 0, 2, &ctx->tokenizer_tiles);
    num("HPGV_STATS_ROWS", 1, 255, &ctx->stats_rows);
    num("HPGV_STATS_BS", 64, 1024, &ctx->stats_bs);
    num("HPGV_STATS_DEBUG", 0, 1, &ctx->stats_debug);
    num("HPGV_FISHER_LDS", 0, 160 * 1024, &ctx->fisher_lds);
    num("HPGV_INFLATE_LDS_PAD", 0, 160 * 1024, &ctx->inflate_lds_pad);
    num("HPGV_INFLATE_WAVE_WGS", 0, 64, &ctx->inflate_wave_wgs);
    num("HPGV_INFLATE_LANE_WGS", 0, 64, &ctx->inflate_lane_wgs);
#endif
}

int hpgv_create(int device_id, hpgv_ctx **out) {
    if (!out) return fail(nullptr, HPGV_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, HPGV_ERR_NO_DEVICE,
                    "no usable HIP device (%s); this engine has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, HPGV_ERR_INVALID, "device_id %d out of range [0,%d)", device_id, n);
    hpgv_ctx *ctx = new (std::nothrow) hpgv_ctx();
    if (!ctx) return fail(nullptr, HPGV_ERR_NOMEM, "out of host memory");
    ctx->device = device_id;
    DeviceGuard g(device_id);
    for (int i = 0; i < 4; ++i) {
        e = hipEventCreate(&ctx->ev[i]);
        if (e != hipSuccess) {
            int rc = fail(nullptr, HPGV_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
            delete ctx;
            return rc;
        }
    }
    hipDeviceProp_t prop;
    memset(&prop, 0, sizeof prop);
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->n_cus = prop.multiProcessorCount;
    ctx->batch_lds_max = hpgv_batch_lds_optin(prop, ctx->batch_lds_max);
    read_environment(ctx);
    e = hipMalloc(&ctx->d_sink, 256);
    if (e != hipSuccess) {
        int rc = fail(nullptr, HPGV_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e));
        delete ctx;
        return rc;
    }
    *out = ctx;
    return HPGV_OK;
}

int hpgv_create_multi(const int *device_ids, int n_devices, hpgv_ctx **out) {
    if (!out) return fail(nullptr, HPGV_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return fail(nullptr, HPGV_ERR_INVALID, "hpgv_create_multi needs 1..64 device ids");
    hpgv_ctx *g = new (std::nothrow) hpgv_ctx();
    if (!g) return fail(nullptr, HPGV_ERR_NOMEM, "out of host memory");
    for (int i = 0; i < n_devices; ++i) {
        hpgv_ctx *m = nullptr;
        const int rc = hpgv_create(device_ids[i], &m);          // the same id twice gives two contexts on one device
        if (rc != HPGV_OK) {
            for (hpgv_ctx *c : g->members) { c->parent = nullptr; hpgv_destroy(c); }
            g->members.clear();
            delete g;
            return rc;                                          // hpgv_last_error(NULL) holds the member's text
        }
        m->parent = g;
        g->members.push_back(m);
    }
    g->device = g->members[0]->device;
    *out = g;
    return HPGV_OK;
}

int hpgv_group_size(const hpgv_ctx *ctx) { return !ctx ? 0 : (is_group(ctx) ? (int)ctx->members.size() : 1); }

hpgv_ctx *hpgv_group_member(hpgv_ctx *ctx, int i) {
    if (!ctx) return nullptr;
    if (!is_group(ctx)) return i == 0 ? ctx : nullptr;
    return (i >= 0 && i < (int)ctx->members.size()) ? ctx->members[(size_t)i] : nullptr;
}

int hpgv_member_device(const hpgv_ctx *ctx, int i) {
    if (!ctx) return -1;
    if (!is_group(ctx)) return i == 0 ? ctx->device : -1;
    return (i >= 0 && i < (int)ctx->members.size()) ? ctx->members[(size_t)i]->device : -1;
}

}  // extern "C"
namespace {
void grow_release(hpgv_ctx::GrowRange &r) {
    size_t off = 0;
    for (size_t i = 0; i < r.pieces.size(); ++i) { (void)hipMemUnmap(r.base + off, r.sizes[i]); (void)hipMemRelease(r.pieces[i]); off += r.sizes[i]; }
    if (r.base) (void)hipMemAddressFree(r.base, r.reserved);
    r = hpgv_ctx::GrowRange();
}
}  // namespace
extern "C" {

void hpgv_destroy(hpgv_ctx *ctx) {
    if (!ctx) return;
    if (is_group(ctx)) {
        hpgv_group_release(ctx);
        for (hpgv_ctx *m : ctx->members) { m->parent = nullptr; hpgv_destroy(m); }
        ctx->members.clear();
        delete ctx;
        return;
    }
    DeviceGuard g(ctx->device);
    (void)hipDeviceSynchronize();
    if (ctx->d_mendel_male) (void)hipFree(ctx->d_mendel_male);
    for (DevBuf *b : {&ctx->d_sg_chunks, &ctx->d_group_of_col, &ctx->d_cond, &ctx->d_perm, &ctx->d_strata, &ctx->d_strata_steps, &ctx->d_cmh_tables, &ctx->d_cov, &ctx->d_lin, &ctx->d_linperm, &ctx->d_linperm_rows, &ctx->d_flips, &ctx->d_flip_tail, &ctx->d_thr, &ctx->assoc.d_cols, &ctx->tdt.d_cols,
                      &ctx->stats.d_cols, &ctx->sgroups.d_cols, &ctx->mendel.d_cols}) b->release();
    ctx->tdt_plan.release();
    if (ctx->d_lf_base) (void)hipFree(ctx->d_lf_base);
    if (ctx->d_sink) (void)hipFree(ctx->d_sink);
    if (ctx->d_crc_tab) (void)hipFree(ctx->d_crc_tab);
    for (auto *t : ctx->tok_scratch) {
        for (DevBuf *b : {&t->blocks, &t->line_off, &t->extra}) b->release();
        delete t;
    }
    ctx->tok_scratch.clear();
    for (auto &r : ctx->grow) grow_release(r);
    ctx->grow.clear();
    hpgv_epi_release(ctx->epi);
    for (Slot *s : ctx->slots) {
        s->release();
        if (s->stream) (void)hipStreamDestroy(s->stream);
        delete s;
    }
    for (int i = 0; i < 4; ++i) if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    delete ctx;
}

// the forms that lost their A/B (profiles/experiments_that_did_not_pay.md) are compiled only with -DHPGV_ABLATION (tools/): the
// shipped library holds one form of each kernel and refuses an option value that names another
#ifdef HPGV_ABLATION
#define HPGV_SHIPPED_ONLY(ok, what)
#else
#define HPGV_SHIPPED_ONLY(ok, what) if (!(ok)) return fail(ctx, HPGV_ERR_UNSUPPORTED, what ": that form is an ablation build's (-DHPGV_ABLATION, tools/build_ablation.py)");
#endif

int hpgv_set_option(hpgv_ctx *ctx, const char *key, long value) {
    if (is_group(ctx) && key && !strcmp(key, "group_self_exchange")) { ctx->group_self_exchange = value ? 1 : 0; return HPGV_OK; }
    if (is_group(ctx) && key && !strcmp(key, "group_fake_ranks")) {
        if (value < 0 || value > 65536) return fail(ctx, HPGV_ERR_INVALID, "group_fake_ranks must be 0 (ranks by distinct device) or the number of members that share rank 0");
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->grp) return fail(ctx, HPGV_ERR_STATE, "group_fake_ranks must be set before the group's communicator exists (hpgv_group_comm_init, the first group call)");
        ctx->group_fake_ranks = value;
        return HPGV_OK;
    }
    GROUP_ALL(ctx, hpgv_set_option(m_, key, value))
    if (!ctx || !key) return HPGV_ERR_INVALID;
    if (!strcmp(key, "row_align")) {
        if (value < 16 || (value & (value - 1))) return fail(ctx, HPGV_ERR_INVALID, "row_align must be a power of two >= 16");
        if (ctx->assoc.set || ctx->tdt.set || ctx->stats.set)
            return fail(ctx, HPGV_ERR_STATE, "row_align must be set before the cohort");
        ctx->row_align = value;
    } else if (!strcmp(key, "row_pad")) {
        if (value < 0 || value % 16 || value > 65536) return fail(ctx, HPGV_ERR_INVALID, "row_pad must be a multiple of 16 in [0, 65536]");
        if (ctx->assoc.set || ctx->tdt.set || ctx->stats.set)
            return fail(ctx, HPGV_ERR_STATE, "row_pad must be set before the cohort");
        ctx->row_pad = value;
    } else if (!strcmp(key, "variants_per_wave")) {
        if (value < 1 || value > 1024) return fail(ctx, HPGV_ERR_INVALID, "variants_per_wave out of range");
        ctx->vpw = value;
    } else if (!strcmp(key, "nontemporal")) {
        HPGV_SHIPPED_ONLY(value != 0, "nontemporal = 0")
        ctx->nontemporal = value ? 1 : 0;
    } else if (!strcmp(key, "profile")) {
        ctx->profile = value ? 1 : 0;
    } else if (!strcmp(key, "scan_unroll")) {
        if (value != 4 && value != 8 && value != 10 && value != 12 && value != 16)
            return fail(ctx, HPGV_ERR_INVALID, "scan_unroll must be one of 4, 8, 10, 12, 16");
        HPGV_SHIPPED_ONLY(value == 4, "scan_unroll other than 4")
        ctx->scan_unroll = value;
    } else if (!strcmp(key, "pipeline")) {
        HPGV_SHIPPED_ONLY(value != 0, "pipeline = 0")
        ctx->pipeline = value ? 1 : 0;
    } else if (!strcmp(key, "fisher_cut_exp")) {
        if (value < 12 || value > 300) return fail(ctx, HPGV_ERR_INVALID, "fisher_cut_exp must be in [12, 300]");
        ctx->fisher_cut_exp = value;
    } else if (!strcmp(key, "epi_complete")) {
        ctx->epi_complete = value ? 1 : 0;
    } else if (!strcmp(key, "epi_triples_mfma")) {
        ctx->epi_triples_mfma = value ? 1 : 0;
    } else if (!strcmp(key, "epi_pairs_mfma")) {
        ctx->epi_pairs_mfma = value ? 1 : 0;
    } else if (!strcmp(key, "epi_wide")) {
        if (value < 0 || value > 2) return fail(ctx, HPGV_ERR_INVALID, "epi_wide must be 0 (the packed kernels' limits), 1 (the wide kernel where the shape needs it) or 2 (the wide kernel for every listed-combination launch)");
        ctx->epi_wide = value;
    } else if (!strcmp(key, "epi_triples_1pass")) {
        if (value < 0 || value > 2) return fail(ctx, HPGV_ERR_INVALID, "epi_triples_1pass must be 0 (two passes), 1 (the cells nine at a time) or 2 (one pass, one wave per SIMD)");
        HPGV_SHIPPED_ONLY(value != 2, "epi_triples_1pass = 2")
        ctx->epi_triples_1pass = value;
    } else if (!strcmp(key, "scan_lds")) {
        if (value < 0 || value > 160 * 1024) return fail(ctx, HPGV_ERR_INVALID, "scan_lds must be in [0, 163840]");
        ctx->scan_lds = value;
    } else if (!strcmp(key, "batch_copy")) {
        ctx->batch_copy = value ? 1 : 0;
    } else if (!strcmp(key, "inflate_wave")) {
        if (value < 0 || value > 4) return fail(ctx, HPGV_ERR_INVALID, "inflate_wave must be 0 (lane per block), 1 (by the number of blocks), 2 (wave per block), 4 (wave per block, several symbols per round) or 3 (lane per block, symbol tables in LDS)");
        HPGV_SHIPPED_ONLY(value == 1 || value == 4, "inflate_wave other than 1 / 4 (a wave per block, several symbols per round)")
        ctx->inflate_wave = value;
    } else if (!strcmp(key, "tokenizer_tiles")) {
        if (value < 0 || value > 2) return fail(ctx, HPGV_ERR_INVALID, "tokenizer_tiles must be 2 (one sweep), 1 (two sweeps) or 0 (line by line)");
        HPGV_SHIPPED_ONLY(value == 1, "tokenizer_tiles other than 1 (two sweeps)")
        ctx->tokenizer_tiles = value;
    } else if (!strcmp(key, "fisher_width")) {
        if (value != 64 && value != 32 && value != 16 && value != 8) return fail(ctx, HPGV_ERR_INVALID, "fisher_width must be 64, 32, 16 or 8");
        HPGV_SHIPPED_ONLY(value == 16, "fisher_width other than 16")
        ctx->fisher_width = value;
    } else if (!strcmp(key, "batch_fused")) {
        ctx->batch_fused = value ? 1 : 0;
    } else if (!strcmp(key, "pipe_waves")) {
        if (value != 4 && value != 6 && value != 8) return fail(ctx, HPGV_ERR_INVALID, "pipe_waves must be 4, 6 or 8");
        HPGV_SHIPPED_ONLY(value == 4, "pipe_waves other than 4")
        ctx->pipe_waves = value;
    } else if (!strcmp(key, "persistent")) {
        HPGV_SHIPPED_ONLY(value == 0, "persistent = 1")
        ctx->persistent = value ? 1 : 0;
    } else if (!strcmp(key, "part_aligned_loads")) {
        HPGV_SHIPPED_ONLY(value == 0, "part_aligned_loads = 1")
        ctx->part_aligned = value ? 1 : 0;
    } else if (!strcmp(key, "pca_apply_vector")) {
        HPGV_SHIPPED_ONLY(value == 0, "pca_apply_vector = 1")
        ctx->pca_apply_vector = value ? 1 : 0;
    } else if (!strcmp(key, "blocks_per_cu")) {
        if (value < 1 || value > 8) return fail(ctx, HPGV_ERR_INVALID, "blocks_per_cu must be in 1..8");
        ctx->blocks_per_cu = value;
    } else {
        return fail(ctx, HPGV_ERR_INVALID, "unknown option '%s'", key);
    }
    return HPGV_OK;
}

/* ---- cohort ---------------------------------------------------------------- */

int hpgv_set_cohort(hpgv_ctx *ctx, const uint8_t *condition, int n_samples) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_cohort(m_, condition, n_samples))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!condition || n_samples < 0) return fail(ctx, HPGV_ERR_INVALID, "bad cohort arguments");
    DeviceGuard g(ctx->device);
    int nA = 0, nU = 0;
    for (int j = 0; j < n_samples; ++j) {
        if (condition[j] == HPGV_COND_AFFECTED) nA++;
        else if (condition[j] == HPGV_COND_UNAFFECTED) nU++;
    }
    size_t segA = round_up((size_t)nA, 16), segU = round_up((size_t)nU, 16);
    size_t pitch = round_up(segA + segU, (size_t)ctx->row_align) + (size_t)ctx->row_pad;
    if (pitch == 0) pitch = (size_t)ctx->row_align;
    if (!pitch_supported(pitch)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "cohort of %d samples exceeds the row-length limit", n_samples);
    Layout &L = ctx->assoc;
    ctx->n_perms = ctx->perm_rows = 0;             // the label rows of hpgv_set_perm_labels belong to the cohort they were given for
    ctx->n_covar = 0;                              // and so do the covariates of hpgv_set_covariates
    ctx->n_strata = ctx->strata_rows = 0;          // and the strata of hpgv_set_strata
    ctx->has_pheno = false; ctx->lin_y.clear(); ctx->lin_cov.clear();      // and the phenotype of hpgv_set_phenotype
    ctx->n_linperms = 0;                           // with the permutations of its residuals (hpgv_set_linear_perms)
    L.n_samples = n_samples;
    L.pitch = pitch;
    L.col_of_pos.assign(pitch, -1);
    size_t a = 0, u = segA;
    for (int j = 0; j < n_samples; ++j) {
        if (condition[j] == HPGV_COND_AFFECTED) L.col_of_pos[a++] = j;
        else if (condition[j] == HPGV_COND_UNAFFECTED) L.col_of_pos[u++] = j;
    }
    ctx->nA = nA; ctx->nU = nU; ctx->chunksA = (int)(segA / 16);
    {   // the conditions themselves, for the kernel that counts in VCF column order with masks (k_assoc_rows)
        std::vector<uint8_t> cond(round_up((size_t)n_samples, 16) + 16, (uint8_t)HPGV_COND_OTHER);
        for (int j = 0; j < n_samples; ++j) cond[(size_t)j] = condition[j] == HPGV_COND_AFFECTED ? 1 : condition[j] == HPGV_COND_UNAFFECTED ? 0 : 2;
        HIPCHK(ctx, ctx->d_cond.reserve(cond.size()));
        HIPCHK(ctx, hipMemcpy(ctx->d_cond.p, cond.data(), cond.size(), hipMemcpyHostToDevice));
    }
    return upload_layout(ctx, L);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_assoc_layout(const hpgv_ctx *ctx, int *n_affected, int *n_unaffected, size_t *pitch) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->assoc.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_cohort has not been called");
    if (n_affected) *n_affected = ctx->nA;
    if (n_unaffected) *n_unaffected = ctx->nU;
    if (pitch) *pitch = ctx->assoc.pitch;
    return HPGV_OK;
}

int hpgv_set_logfact(hpgv_ctx *ctx, const double *table, size_t n) {
    GROUP_ALL(ctx, hpgv_set_logfact(m_, table, n))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!table || n == 0) return fail(ctx, HPGV_ERR_INVALID, "empty log-factorial table");
    DeviceGuard g(ctx->device);
    ctx->n_lf = 0;
    if (ctx->cap_lf < n) {
        // two doubles of padding in front and behind: the Fisher pass reads the table two entries per load, and the neighbour
        // of a term at the edge of its support may be entry -1 or n (read, never used)
        if (ctx->d_lf_base) { (void)hipFree(ctx->d_lf_base); ctx->d_lf_base = nullptr; ctx->d_lf = nullptr; ctx->cap_lf = 0; }
        HIPCHK(ctx, hipMalloc(&ctx->d_lf_base, (n + 4) * sizeof(double)));
        HIPCHK(ctx, hipMemset(ctx->d_lf_base, 0, (n + 4) * sizeof(double)));
        ctx->d_lf = ctx->d_lf_base + 2;
        ctx->cap_lf = n;
    }
    HIPCHK(ctx, hipMemcpy(ctx->d_lf, table, n * sizeof(double), hipMemcpyHostToDevice));
    ctx->n_lf = n;
    return HPGV_OK;
}

int hpgv_set_stats_cohort(hpgv_ctx *ctx, int n_samples) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_stats_cohort(m_, n_samples))
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_samples < 0) return fail(ctx, HPGV_ERR_INVALID, "negative n_samples");
    DeviceGuard g(ctx->device);
    size_t pitch = round_up(round_up((size_t)n_samples, 16), (size_t)ctx->row_align);
    if (pitch == 0) pitch = (size_t)ctx->row_align;
    if (!pitch_supported(pitch)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "cohort of %d samples exceeds the row-length limit", n_samples);
    Layout &L = ctx->stats;
    L.n_samples = n_samples;
    L.pitch = pitch;
    L.col_of_pos.assign(pitch, -1);
    for (int j = 0; j < n_samples; ++j) L.col_of_pos[j] = j;
    return upload_layout(ctx, L);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_set_stats_groups(hpgv_ctx *ctx, const int32_t *group_of_sample, int n_samples, int n_groups) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_stats_groups(m_, group_of_sample, n_samples, n_groups))
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_samples < 0 || n_groups < 1 || n_groups > 4096 || (n_samples > 0 && !group_of_sample))
        return fail(ctx, HPGV_ERR_INVALID, "bad stats group arguments");
    DeviceGuard g(ctx->device);
    std::vector<int> size((size_t)n_groups, 0);
    for (int j = 0; j < n_samples; ++j) {
        if (group_of_sample[j] >= n_groups) return fail(ctx, HPGV_ERR_INVALID, "group %d of sample %d out of range", group_of_sample[j], j);
        if (group_of_sample[j] >= 0) size[(size_t)group_of_sample[j]]++;
    }
    std::vector<uint32_t> off((size_t)n_groups, 0);
    size_t used = 0;
    for (int k = 0; k < n_groups; ++k) { off[(size_t)k] = (uint32_t)used; used += round_up((size_t)size[(size_t)k], 16); }
    size_t pitch = round_up(used, (size_t)ctx->row_align) + (size_t)ctx->row_pad;
    if (pitch == 0) pitch = (size_t)ctx->row_align;
    if (!pitch_supported(pitch)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "cohort of %d samples exceeds the row-length limit", n_samples);
    Layout &L = ctx->sgroups;
    L.n_samples = n_samples;
    L.pitch = pitch;
    L.col_of_pos.assign(pitch, -1);
    std::vector<size_t> fill(off.begin(), off.end());
    for (int j = 0; j < n_samples; ++j)
        if (group_of_sample[j] >= 0) L.col_of_pos[fill[(size_t)group_of_sample[j]]++] = j;
    ctx->sg_off = off;
    ctx->sg_size = size;
    {   // first chunk / chunk count per group for the one-pass stats kernel
        std::vector<int32_t> tab((size_t)n_groups * 2);
        for (int k = 0; k < n_groups; ++k) {
            tab[(size_t)k] = (int32_t)(off[(size_t)k] / 16);
            tab[(size_t)n_groups + (size_t)k] = (int32_t)(round_up((size_t)size[(size_t)k], 16) / 16);
        }
        HIPCHK(ctx, ctx->d_sg_chunks.reserve(tab.size() * sizeof(int32_t)));
        HIPCHK(ctx, hipMemcpy(ctx->d_sg_chunks.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    {   // the group of every column, for the kernel that counts groups with masks over the columns in VCF order (k_stats_all2)
        std::vector<uint8_t> gid(round_up((size_t)n_samples, 16) + 16, 0xFF);
        bool all = n_samples > 0;
        for (int j = 0; j < n_samples; ++j) {
            if (group_of_sample[j] >= 0 && group_of_sample[j] < 255) gid[(size_t)j] = (uint8_t)group_of_sample[j];
            else all = false;
        }
        ctx->all_grouped = all;
        HIPCHK(ctx, ctx->d_group_of_col.reserve(gid.size()));
        HIPCHK(ctx, hipMemcpy(ctx->d_group_of_col.p, gid.data(), gid.size(), hipMemcpyHostToDevice));
    }
    return upload_layout(ctx, L);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_stats_groups_layout(const hpgv_ctx *ctx, size_t *pitch, int *group_sizes) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->sgroups.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_groups has not been called");
    if (pitch) *pitch = ctx->sgroups.pitch;
    if (group_sizes) for (size_t k = 0; k < ctx->sg_size.size(); ++k) group_sizes[k] = ctx->sg_size[k];
    return HPGV_OK;
}

int hpgv_stats_layout(const hpgv_ctx *ctx, size_t *pitch) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->stats.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_stats_cohort has not been called");
    if (pitch) *pitch = ctx->stats.pitch;
    return HPGV_OK;
}

int hpgv_set_families(hpgv_ctx *ctx, int n_samples, int n_families, const int32_t *father_col,
                      const int32_t *mother_col, const int32_t *child_off, const int32_t *child_col,
                      const uint8_t *child_sex) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_families(m_, n_samples, n_families, father_col, mother_col, child_off, child_col, child_sex))
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_samples < 0 || n_families < 0 || (n_families > 0 && (!father_col || !mother_col || !child_off)))
        return fail(ctx, HPGV_ERR_INVALID, "bad family arguments");
    DeviceGuard g(ctx->device);
    Layout &L = ctx->tdt;
    ctx->n_flips = ctx->flip_rows = ctx->flip_pitch = 0;      // the flip rows of hpgv_set_tdt_flips belong to the families they were given for
    std::string why;
    int rc = ctx->tdt_plan.build(n_samples, n_families, father_col, mother_col, child_off, child_col,
                                 child_sex, (size_t)ctx->row_align, L.col_of_pos, L.pitch, why);
    if (rc != HPGV_OK) return fail(ctx, rc, "%s", why.c_str());
    if (!pitch_supported(L.pitch)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "pedigree exceeds the row-length limit");
    L.n_samples = n_samples;
    ctx->tdt_families = n_families;
    return upload_layout(ctx, L);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_set_pedigree(hpgv_ctx *ctx, int n_samples, int n_trios, const int32_t *father_col, const int32_t *mother_col,
                      const int32_t *child_col, const uint8_t *child_sex) {
    HPGV_ABI_TRY
    GROUP_ALL(ctx, hpgv_set_pedigree(m_, n_samples, n_trios, father_col, mother_col, child_col, child_sex))
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_samples < 0 || n_trios < 0 || (n_trios > 0 && (!father_col || !mother_col || !child_col || !child_sex)))
        return fail(ctx, HPGV_ERR_INVALID, "bad pedigree arguments");
    for (int t = 0; t < n_trios; ++t)
        if (father_col[t] < 0 || father_col[t] >= n_samples || mother_col[t] < 0 || mother_col[t] >= n_samples ||
            child_col[t] < 0 || child_col[t] >= n_samples)
            return fail(ctx, HPGV_ERR_INVALID, "trio %d has a column out of range", t);
    DeviceGuard g(ctx->device);
    const size_t P16 = round_up((size_t)n_trios, 16);
    size_t pitch = round_up(3 * P16, (size_t)ctx->row_align) + (size_t)ctx->row_pad;
    if (pitch == 0) pitch = (size_t)ctx->row_align;
    if (!pitch_supported(pitch)) return fail(ctx, HPGV_ERR_UNSUPPORTED, "pedigree exceeds the row-length limit");
    Layout &L = ctx->mendel;
    L.n_samples = n_samples;
    L.pitch = pitch;
    L.col_of_pos.assign(pitch, -1);
    std::vector<uint8_t> male(P16 ? P16 : 16, 0);
    for (int t = 0; t < n_trios; ++t) {
        L.col_of_pos[(size_t)t] = father_col[t];
        L.col_of_pos[P16 + (size_t)t] = mother_col[t];
        L.col_of_pos[2 * P16 + (size_t)t] = child_col[t];
        male[(size_t)t] = child_sex[t] == HPGV_SEX_MALE ? 0xFF : 0x00;
    }
    if (ctx->d_mendel_male) { (void)hipFree(ctx->d_mendel_male); ctx->d_mendel_male = nullptr; }
    HIPCHK(ctx, hipMalloc(&ctx->d_mendel_male, male.size()));
    HIPCHK(ctx, hipMemcpy(ctx->d_mendel_male, male.data(), male.size(), hipMemcpyHostToDevice));
    hpgv::mendel_host::build_luts(ctx->mendel_luts);
    ctx->mendel_trios = n_trios;
    ctx->mendel_pchunks = (int)(P16 / 16);
    return upload_layout(ctx, L);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_mendel_layout(const hpgv_ctx *ctx, size_t *pitch) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->mendel.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_pedigree has not been called");
    if (pitch) *pitch = ctx->mendel.pitch;
    return HPGV_OK;
}

int hpgv_tdt_layout(const hpgv_ctx *ctx, int *n_trios_fast, int *n_families_slow, size_t *pitch) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!ctx->tdt.set) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_families has not been called");
    if (n_trios_fast) *n_trios_fast = ctx->tdt_plan.n_fast;
    if (n_families_slow) *n_families_slow = ctx->tdt_plan.n_slow_families;
    if (pitch) *pitch = ctx->tdt.pitch;
    return HPGV_OK;
}

/* ---- memory ---------------------------------------------------------------- */

int hpgv_dev_alloc(hpgv_ctx *ctx, size_t bytes, void **dptr) {
    ctx = first_member(ctx);
    if (!ctx || !dptr) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    HIPCHK(ctx, hipMalloc(dptr, bytes ? bytes : 16));
    return HPGV_OK;
}
int hpgv_dev_free(hpgv_ctx *ctx, void *dptr) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    if (dptr) HIPCHK(ctx, hipFree(dptr));
    return HPGV_OK;
}
// Device memory that grows in place: an address range is reserved (costs nothing), and backed piece by piece as the caller
// learns how much it needs -- a bgzip file's text, whose size is only known when its last block header has been seen.  The
// range behaves like any device pointer (kernels, copies).  HPGV_ERR_UNSUPPORTED when the device has no virtual memory management.
// the allocation granularity of the device's virtual memory management, as a multiple of it that is at least `at_least`
static size_t vmm_granularity(int device, size_t at_least) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = device;
    size_t g = 0;
    if (hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || g == 0) { (void)hipGetLastError(); g = (size_t)2 << 20; }
    return (at_least + g - 1) / g * g;
}
int hpgv_dev_reserve(hpgv_ctx *ctx, size_t max_bytes, void **dptr) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx || !dptr || !max_bytes) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    int vmm = 0;
    if (hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, ctx->device) != hipSuccess || !vmm)
        return fail(ctx, HPGV_ERR_UNSUPPORTED, "the device has no virtual memory management");
    const size_t gran = vmm_granularity(ctx->device, (size_t)2 << 20);      // what the device asks for, at least 2 MB
    hpgv_ctx::GrowRange r;
    r.reserved = (max_bytes + gran - 1) / gran * gran;
    void *p = nullptr;
    HIPCHK(ctx, hipMemAddressReserve(&p, r.reserved, gran, nullptr, 0));
    r.base = (char *)p;
    { std::lock_guard<std::mutex> lk(ctx->mu); ctx->grow.push_back(r); }
    *dptr = p;
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}
// makes the range's first `bytes` bytes usable (a no-op when they are already); what is backed stays backed -- also the pieces
// a failing call mapped before it failed: hpgv_dev_committed says how far the range is backed
int hpgv_dev_commit(hpgv_ctx *ctx, void *dptr, size_t bytes) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx || !dptr) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto &r : ctx->grow) {
        if (r.base != (char *)dptr) continue;
        if (bytes <= r.committed) return HPGV_OK;
        if (bytes > r.reserved) return fail(ctx, HPGV_ERR_INVALID, "commit of %zu bytes in a range of %zu", bytes, r.reserved);
        const size_t gran = vmm_granularity(ctx->device, (size_t)64 << 20);      // pieces of 64 MB, rounded to the device's granularity
        size_t add = (bytes - r.committed + gran - 1) / gran * gran;
        if (r.committed + add > r.reserved) add = r.reserved - r.committed;
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = ctx->device;
        hipMemAccessDesc acc = {};
        acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
        // one piece for all of it; should the runtime refuse that, pieces of 64 MB
        hipError_t last = hipSuccess;
        for (size_t piece = add; add > 0; piece = gran) {
            while (add > 0) {
                const size_t n = piece < add ? piece : add;
                hipMemGenericAllocationHandle_t h;
                const bool trace = ctx->vmm_trace != 0;
                last = hipMemCreate(&h, n, &prop, 0);
                if (trace) fprintf(stderr, "vmm: create %zu MB: %s\n", n >> 20, hipGetErrorString(last));
                if (last != hipSuccess) break;
                last = hipMemMap(r.base + r.committed, n, 0, h, 0);
                if (trace) fprintf(stderr, "vmm: map at +%zu MB (%p): %s\n", r.committed >> 20, (void *)(r.base + r.committed), hipGetErrorString(last));
                if (last == hipSuccess) {
                    // access is set for EVERYTHING backed so far, not for the new piece alone: the runtime (ROCm 7.2) refuses the
                    // third and later pieces of a reservation when it is asked piece by piece ("invalid argument", eleven
                    // times out of twelve; tools/exp/vmm_seq.py), and never this form
                    last = hipMemSetAccess(r.base, r.committed + n, &acc, 1);
                    if (trace) fprintf(stderr, "vmm: set-access: %s\n", hipGetErrorString(last));
                    if (last != hipSuccess) (void)hipMemUnmap(r.base + r.committed, n);
                }
                if (last != hipSuccess) { (void)hipMemRelease(h); break; }
                r.pieces.push_back(h); r.sizes.push_back(n); r.committed += n; add -= n;
            }
            if (add == 0 || piece == gran) break;
            (void)hipGetLastError();
        }
        if (add > 0) return fail(ctx, HPGV_ERR_NOMEM, "mapping device memory (%zu bytes short): %s", add, hipGetErrorString(last));
        return HPGV_OK;
    }
    return fail(ctx, HPGV_ERR_INVALID, "not a range of hpgv_dev_reserve");
    HPGV_ABI_CATCH(ctx)
}
int hpgv_dev_committed(hpgv_ctx *ctx, void *dptr, size_t *bytes) {
    ctx = first_member(ctx);
    if (!ctx || !dptr || !bytes) return HPGV_ERR_INVALID;
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (auto &r : ctx->grow) if (r.base == (char *)dptr) { *bytes = r.committed; return HPGV_OK; }
    return fail(ctx, HPGV_ERR_INVALID, "not a range of hpgv_dev_reserve");
}
int hpgv_dev_release(hpgv_ctx *ctx, void *dptr) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (!dptr) return HPGV_OK;
    DeviceGuard g(ctx->device);
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (size_t i = 0; i < ctx->grow.size(); ++i)
        if (ctx->grow[i].base == (char *)dptr) { grow_release(ctx->grow[i]); ctx->grow.erase(ctx->grow.begin() + (long)i); return HPGV_OK; }
    return fail(ctx, HPGV_ERR_INVALID, "not a range of hpgv_dev_reserve");
    HPGV_ABI_CATCH(ctx)
}
// NUMA node the device hangs off (sysfs numa_node of its PCI function), -1 when the system does not say: a host that
// stages batches for the device does best with its staging threads and page-locked buffers on that node
int hpgv_device_numa_node(hpgv_ctx *ctx, int *node) {
    ctx = first_member(ctx);
    if (!ctx || !node) return HPGV_ERR_INVALID;
    *node = -1;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, ctx->device) != hipSuccess) return HPGV_OK;
    for (char *c = bus; *c; ++c) *c = (char)tolower((unsigned char)*c);
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE *f = fopen(path, "r")) {
        int n = -1;
        if (fscanf(f, "%d", &n) == 1) *node = n;
        fclose(f);
    }
    return HPGV_OK;
}
// a stream of the caller's own (non-blocking), e.g. for copies that should overlap the engine's work
int hpgv_stream_create(hpgv_ctx *ctx, void **stream) {
    ctx = first_member(ctx);
    if (!ctx || !stream) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    hipStream_t st = nullptr;
    HIPCHK(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = (void *)st;
    return HPGV_OK;
}
// a stream whose kernels give way to those of the other streams whenever the device has a choice (bulk work beside a pipeline)
int hpgv_stream_create_low(hpgv_ctx *ctx, void **stream) {
    ctx = first_member(ctx);
    if (!ctx || !stream) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    int least = 0, greatest = 0;
    HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t st = nullptr;
    HIPCHK(ctx, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, least));
    *stream = (void *)st;
    return HPGV_OK;
}
int hpgv_stream_destroy(hpgv_ctx *ctx, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    if (stream) HIPCHK(ctx, hipStreamDestroy((hipStream_t)stream));
    return HPGV_OK;
}
// "the text at host_text is already on the device at d_text": the *_text entry points then tokenize d_text in place
// instead of copying host_text over (d_text = NULL takes the entry away).  For readers that produce the text on the
// device (hpgv_inflate_blocks_dev) and keep a host copy for the result writers.
int hpgv_memset_dev(hpgv_ctx *ctx, void *dptr, int byte_value, size_t bytes, void *stream) {
    ctx = first_member(ctx);
    if (!ctx || (bytes > 0 && !dptr)) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    if (stream) HIPCHK(ctx, hipMemsetAsync(dptr, byte_value, bytes, (hipStream_t)stream));
    else HIPCHK(ctx, hipMemset(dptr, byte_value, bytes));
    return HPGV_OK;
}
int hpgv_text_alias(hpgv_ctx *ctx, const char *host_text, const char *d_text) {
    ctx = first_member(ctx);
    if (!ctx || !host_text) return HPGV_ERR_INVALID;
    std::lock_guard<std::mutex> lk(ctx->alias_mu);
    for (size_t i = 0; i < ctx->text_alias.size(); ++i)
        if (ctx->text_alias[i].first == host_text) {
            const char *old = ctx->text_alias[i].second;
            for (size_t k = 0; k < ctx->text_tiles.size(); ++k) if (ctx->text_tiles[k].d_text == old) { ctx->text_tiles.erase(ctx->text_tiles.begin() + (long)k); break; }
            ctx->text_alias.erase(ctx->text_alias.begin() + (long)i);
            break;
        }
    if (d_text) ctx->text_alias.emplace_back(host_text, d_text);
    return HPGV_OK;
}
int hpgv_text_alias_tiles(hpgv_ctx *ctx, const char *host_text, const char *d_text, const char *d_text_base, const void *d_tiles, uint64_t n_tiles) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx || !host_text) return HPGV_ERR_INVALID;
    if (d_text && d_tiles && (!d_text_base || d_text < d_text_base)) return fail(ctx, HPGV_ERR_INVALID, "the window lies in front of its text");
    std::lock_guard<std::mutex> lk(ctx->alias_mu);
    const char *old = nullptr;
    for (size_t i = 0; i < ctx->text_alias.size(); ++i)
        if (ctx->text_alias[i].first == host_text) { old = ctx->text_alias[i].second; ctx->text_alias.erase(ctx->text_alias.begin() + (long)i); break; }
    for (size_t i = 0; i < ctx->text_tiles.size(); ++i)
        if (ctx->text_tiles[i].d_text == (d_text ? d_text : old)) { ctx->text_tiles.erase(ctx->text_tiles.begin() + (long)i); break; }
    if (d_text) {
        ctx->text_alias.emplace_back(host_text, d_text);
        if (d_tiles && n_tiles > 0) ctx->text_tiles.push_back({d_text, d_text_base, d_tiles, n_tiles});
    }
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}
}  // extern "C"
bool tiles_of_device_text(hpgv_ctx *ctx, const char *d_text, hpgv_ctx::TextTiles *out) {
    std::lock_guard<std::mutex> lk(ctx->alias_mu);
    for (const auto &t : ctx->text_tiles) if (t.d_text == d_text) { *out = t; return true; }
    return false;
}
const char *text_on_device(hpgv_ctx *ctx, const char *host_text) {
    std::lock_guard<std::mutex> lk(ctx->alias_mu);
    for (const auto &a : ctx->text_alias) if (a.first == host_text) return a.second;
    return nullptr;
}
// the member of a group on whose device `host_text` has been declared resident (hpgv_text_alias), or nullptr
hpgv_ctx *alias_owner(hpgv_ctx *group, const char *host_text) {
    for (hpgv_ctx *m : group->members) if (text_on_device(m, host_text)) return m;
    return nullptr;
}
extern "C" {
int hpgv_host_alloc(hpgv_ctx *ctx, size_t bytes, void **hptr) {
    ctx = first_member(ctx);
    if (!ctx || !hptr) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    // visible to every device of a group.  (experiment: HPGV_PINNED_NONCOHERENT=1 -- no difference measured, profiles/experiments_that_did_not_pay.md)
    const unsigned flags = hipHostMallocPortable | (ctx->pinned_noncoherent ? hipHostMallocNonCoherent : 0u);
    HIPCHK(ctx, hipHostMalloc(hptr, bytes ? bytes : 16, flags));
    return HPGV_OK;
}
int hpgv_host_free(hpgv_ctx *ctx, void *hptr) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    if (hptr) HIPCHK(ctx, hipHostFree(hptr));
    return HPGV_OK;
}
int hpgv_memcpy_h2d(hpgv_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return HPGV_OK;
}
// the copy is only queued (page-locked source): hpgv_stream_sync says when it is done
int hpgv_memcpy_h2d_async(hpgv_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return HPGV_OK;
}
int hpgv_memcpy_d2h(hpgv_ctx *ctx, void *dst, const void *src, size_t bytes, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return HPGV_OK;
}
int hpgv_stream_sync(hpgv_ctx *ctx, void *stream) {
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    DeviceGuard g(ctx->device);
    HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
    return HPGV_OK;
}

}  // extern "C"
