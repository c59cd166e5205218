// hpgv_internal.h -- the context behind include/hpgv.h and the helpers shared by the translation units of
// libhpgv.so: hpgv_capi.hip (contexts, options, cohorts, memory, streams, text aliases), hpgv_scan_capi.hip (the
// device-resident *_dev launchers), hpgv_text_capi.hip (tokenizer, the text entry points' front half),
// hpgv_tool_capi.hip (per-batch and text entry points), hpgv_lines_capi.hip (partition / multisplit of lines), and the
// units whose kernel instantiations compile on their own (hpgv_perm_capi.hip, hpgv_ld_capi.hip, hpgv_ibs_capi.hip, hpgv_grm_capi.hip, hpgv_pca_capi.hip, hpgv_logistic_capi.hip, hpgv_cmh_capi.hip, hpgv_linear_capi.hip, hpgv_epi_capi.hip, hpgv_epi_generic_capi.hip, hpgv_statsall_capi.hip, hpgv_inflate_capi.hip, hpgv_group_capi.hip).
// A synchronous entry point has two halves that meet in a Staged: the front puts the call's matrix on the device -- text_front /
// text_front_skip for a text, stage_chain for a host batch that goes through the kernel chain -- and the tool's back half takes it
// from there; the permutation calls build theirs from the halves of hpgv_assoc's and hpgv_tdt's (assoc_chain, ..., below).
// The host side the epistasis units share is in hpgv_epi_host.h.
#pragma once
#include "../../include/hpgv.h"
#include "hpgv_kernels.h"
#include "hpgv_tdt_stats_kernels.h"
#include "hpgv_epi_kernels.h"

#include <hip/hip_runtime.h>
#include <cctype>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace { thread_local std::string g_create_error; }

// a device allocation that only ever grows: kept while it is large enough (hipFree waits for every stream of the device), freed
// and allocated anew when it is not -- what it held does not survive that
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;                    // bytes behind p
    template <typename T = void> T *as() const { return static_cast<T *>(p); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // room for `bytes`: a block too small is replaced by one of `alloc` bytes -- the site's slack rule; less than `bytes` (the
    // default) means exactly `bytes`
    hipError_t reserve(size_t bytes, size_t alloc = 0) {
        if (cap >= bytes) return hipSuccess;
        release();
        const size_t want = alloc > bytes ? alloc : bytes;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    // the same for a block that work queued on `busy` may still use: the stream is waited for before the block is freed
    hipError_t reserve_after_sync(hipStream_t busy, size_t bytes, size_t alloc = 0) {
        if (cap >= bytes) return hipSuccess;
        if (p) { const hipError_t e = hipStreamSynchronize(busy); if (e != hipSuccess) return e; }
        return reserve(bytes, alloc);
    }
    // the slots' rule: a quarter more than asked for, in whole 256 bytes
    hipError_t reserve_slack(size_t bytes) { return reserve(bytes, (bytes + bytes / 4 + 255) / 256 * 256); }
};

// its page-locked twin: host memory (h) the device reads and writes in place (d); half more than asked for, in whole 4 KiB
struct PinnedBuf {
    void *h = nullptr, *d = nullptr;
    size_t cap = 0;
    void release() { if (h) (void)hipHostFree(h); h = d = nullptr; cap = 0; }
    hipError_t reserve(size_t bytes) {
        if (cap >= bytes) return hipSuccess;
        release();
        const size_t want = (bytes + bytes / 2 + 4095) / 4096 * 4096;
        hipError_t e = hipHostMalloc(&h, want, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
        if (e == hipSuccess) cap = want;
        return e;
    }
};

struct Layout {
    bool set = false;
    int n_samples = 0;
    size_t pitch = 0;
    int chunks = 0;
    std::vector<int32_t> col_of_pos;   // size pitch; -1 = pad
    DevBuf d_cols;                     // col_of_pos on the device
    const int32_t *d_col_of_pos() const { return d_cols.as<int32_t>(); }
};

// per-call scratch of the synchronous host entry points: one grow-only buffer per role.  A call reserves the ones it uses; what
// they hold ends with the call -- but for `text` and `meta` under a hold (hpgv_ctx::TextHeld), which keeps the whole slot
struct Slot {
    bool busy = false;
    hipStream_t stream = nullptr;
    // the call's matrix (Staged)
    DevBuf text;       // the host text of a *_text call, of hpgv_tokenize or of hpgv_bgzf_compress
    DevBuf raw;        // genotype rows in VCF column order: the copy of a batch, or what the tokenizer wrote
    DevBuf laid;       // the rows in a tool's layout (HPGV_LAYOUT_*); the record filters and the kernel chain lay out into it in turn
    DevBuf isx;        // per row: on chromosome X
    DevBuf status;     // per line of a text: the tokenizer's status
    DevBuf meta;       // a text's n_lines, line offsets and field offsets (TextMeta)
    // the tools' results on their way out
    DevBuf tally;      // integer counters per row: allele counts, transmission counts, counts8.  The count filters' counts8 and
                       // verdict bytes come first; record_filters has them on the host (its sync) before a tool's tallies follow
    DevBuf dbl;        // doubles per row: odds, chi-square, p; Hardy-Weinberg
    DevBuf gtally;     // the kernel chain's counts8 per phenotype group and row
    DevBuf gdbl;       // their Hardy-Weinberg doubles
    DevBuf ints;       // the allele counts as four arrays, for the copies into the caller's
    DevBuf smiss;      // missing genotypes per sample (the one-pass kernel's child errors per trio behind them)
    DevBuf merr;       // Mendelian errors per row, then child errors per trio: the Mendel filter's, on the host when record_filters
                       // returns (its sync), then the kernel chain's
    DevBuf inherit;    // the inheritance filter's counts8 and verdict bytes
    DevBuf multi;      // multi-allelic rows: their indices, then their 256-bin tables
    DevBuf row_cnt;    // k_stats_all2's per-row counters between its two kernels
    DevBuf perm;       // the permutation call's results and scratch: perm_plan (hpgv_perm_capi.hip) is the one place that knows where its
                       // parts lie.  (hpgv_ld_text has no permutation: its rows' skip bytes lie at the front)
    PinnedBuf res;     // result block of the one-pass kernels (they store into it), staging of k_assoc_rows' results
    // a buffer under two names holds two things that no call has at once:
    DevBuf &heads = text;      // a text that lies on the device already (hpgv_text_alias) is not uploaded: its head offsets and heads
    DevBuf &parts = laid;      // the line tools run on a held text, after its matrix is done with: the partition's / split's output,
    DevBuf &members = isx;     //   the BGZF members made of it (and of hpgv_bgzf_compress's text),
    DevBuf &aux = tally;       //   offsets scratch, keep / bucket bytes, segment tables,
    DevBuf &dfl = dbl;         //   the deflate kernels' scratch
    void release() {
        for (DevBuf *b : {&text, &raw, &laid, &isx, &status, &meta, &tally, &dbl, &gtally, &gdbl, &ints, &smiss, &merr, &inherit, &multi, &row_cnt, &perm}) b->release();
        res.release();
    }
};

// where the tokenizer's outputs per text lie in Slot::meta: n_lines, the starts of max_lines + 1 lines and the text's end, ten field
// offsets per line
struct TextMeta {
    char *base;
    size_t max_lines;
    TextMeta(const DevBuf &meta, int max_lines_) : base(meta.as<char>()), max_lines((size_t)max_lines_) {}
    static size_t bytes(int max_lines) { return 16 + ((size_t)max_lines + 2) * sizeof(uint64_t) + (size_t)max_lines * 10 * sizeof(uint32_t) + 16; }
    int *n_lines() const { return (int *)base; }
    unsigned long long *line_off() const { return (unsigned long long *)(base + 16); }
    uint32_t *field_off() const { return (uint32_t *)(base + 16 + (max_lines + 2) * sizeof(uint64_t)); }
};

// the genotype matrix of one synchronous call once it is on the device: what the back halves of hpgv_tool_capi.hip,
// hpgv_perm_capi.hip, hpgv_ld_capi.hip, hpgv_ibs_capi.hip and hpgv_grm_capi.hip read, whether a batch (batch_sources / stage_chain) or a text (text_front,
// hpgv_text_capi.hip) put it there
struct Staged {
    const uint8_t *d_raw = nullptr;   // VCF column order: the slot's `raw`, or the caller's rows where the device can read them
    size_t raw_pitch = 0;
    const uint8_t *d_laid = nullptr;  // the slot's `laid` in layout `which`; null when a one-pass kernel reads d_raw itself
    int which = 0;                    // HPGV_LAYOUT_* of d_laid (laid_as keeps both current when the chain lays out anew)
    const uint8_t *d_isx = nullptr;
    int n = 0;                        // rows
    size_t out_stride = 0;            // stride of the per-group outputs: n_variants (batch), max_lines (text)
    bool text = false;                // the tokenizer wrote d_raw: the only matrix k_assoc_rows is run on
};

// epistasis / MDR state: the vcf2epi dataset on the device, its bit planes for the current folds
struct EpiState {
    bool have_data = false, have_folds = false;
    int V = 0, nA = 0, nU = 0, num_folds = 0, W = 0, V_alloc = 0, n_chunks = 0;
    bool wide_only = false;           // the layout has more than EPI_MAX_FOLDS folds or a (fold, class) group of 65 536 samples or more (option "epi_wide"): planes and
                                      // d_group_w0 only -- no marginals, swapped copy or staging chunks; every launch is k_epi_combs_wide
    int fold_cap = 0;                 // fold slots of the layout's tables (group_size, d_folds; the ranking's thresholds and counters): max(num_folds, EPI_MAX_FOLDS)
    int rank_fold_cap = 0;            // fold slots behind d_thr and d_cand_count
    uint8_t *d_data = nullptr;
    uint32_t *d_planes = nullptr;
    uint32_t rev_off = 0;             // words from the planes to their copy with bits 0 and 2 of every nibble swapped (epm_swap02; 0: no copy, the matrix-core scans do not run)
    hpgv_epi_rank_info rank_info{};   // what the last ranking call ran (hpgv_epi_last_rank_info): set where the launches decide
    uint32_t *d_marg = nullptr;       // per SNP and (fold, class) group: samples with genotype 0 / 1 (16 bits each)
    bool complete = false;            // the dataset holds no call other than 0 / 1 / 2
    hpgv::EpiChunk *d_chunks = nullptr;
    uint32_t *d_chunk_cls = nullptr;  // per staging block: bit k = its step k holds controls
    hpgv::EpiFold *d_folds = nullptr;
    uint32_t *d_group_w0 = nullptr;
    std::vector<int32_t> group_size;
    DevBuf cand;                      // the pair and triple rankings' candidate lists (EpiCand / EpiCand3), kept between calls and only ever grown
    unsigned *d_cand_count = nullptr;
    unsigned cand_cap = 0;            // records per fold's list in the current ranking call
    double *d_thr = nullptr;
    DevBuf tile_base;                 // unsigned: the tile tables of a launch
};

struct hpgv_ctx {
    // ---- a GROUP context (hpgv_create_multi) has members and nothing else: one ordinary context per device.  Cohort
    // calls go to every member, the synchronous per-batch calls to the member with the fewest calls in flight, the
    // device-resident calls to member 0; a member's failure text is copied to its group.
    std::vector<hpgv_ctx *> members;
    hpgv_ctx *parent = nullptr;
    struct GroupState *grp = nullptr;   // streams, scratch and the RCCL communicator of the group-wide resident scans (hpgv_group_capi.hip)
    long group_self_exchange = 0;       // test switch: member 0 also hands its results over through the communicator (send / recv to itself)
    long group_fake_ranks = 0;          // test switch, read in comm_setup only: n >= 1 = the first n members share rank 0, every later member is a rank of its own
    std::atomic<unsigned> deal_next{0};
    std::atomic<int> in_flight{0};
    int device = 0;
    mutable std::string err;
    std::mutex mu;
    // options
    long row_align = 16;
    long row_pad = 0;          // extra bytes (multiple of 16) appended to every row; pitch exploration knob
    long vpw = 2;
    long nontemporal = 1;
    long profile = 0;
    std::mutex alias_mu;
    std::vector<std::pair<const char *, const char *>> text_alias;   // host text buffer -> the same text already on the device
    struct TextTiles { const char *d_text, *d_base; const void *d_tiles; uint64_t n_tiles; };
    std::vector<TextTiles> text_tiles;                               // device windows whose text comes with the decoder's tile records (hpgv_text_alias_tiles)
    // hpgv_filter_text keeps its slot -- the device text it tokenized and that text's line starts -- until hpgv_text_partition
    struct TextHeld { const char *host_text; Slot *slot; const char *d_text; const unsigned long long *d_line_off; int n_lines; };
    std::vector<TextHeld> text_held;                                 // (under alias_mu)
    long part_aligned = 0;     // hpgv_lines_partition_dev: 0 = unaligned dwordx4 loads of the source; 1 = aligned loads + v_alignbyte (ablation build)
    long pca_apply_vector = 0; // hpgv_pca_apply_dev: 0 = k_pca_apply on the f64 MFMA; 1 = the lane-per-row v_fma_f64 form (ablation build)
    long scan_unroll = 4;
    long persistent = 0;       // 0: one wave per vpw consecutive rows; 1: persistent strided grid
    long blocks_per_cu = 8;
    long pipeline = 1;         // 1: software-pipelined scan (loads of the next tile before counting this one)
    long pipe_waves = 4;       // register budget of the pipelined scan, as waves per SIMD (4, 6 or 8)
    long fisher_cut_exp = 22;  // Fisher tails stop after a round whose terms are all below 10^-this of the tail's largest term
    long epi_complete = 1;     // epistasis pair scan on a dataset without missing calls: count four cells, derive the other five
    long epi_pairs_mfma = 1;   // epistasis pair ranking, any fold count, data with or without missing calls: cell counts on the matrix cores (k_epi_pairs_mfma) while
                               // both classes stay below 65 536 samples, the samples fit EPM_MAX_CHUNKS staging chunks and the planes' swapped copy exists (rev_off); 0 = k_epi_pairs
    long epi_triples_mfma = 1; // epistasis triple ranking, any fold count: cell counts on the matrix cores (k_epi_triples_mfma) under the same three conditions; 0 = the vector-ALU scans below
    long epi_wide = 0;         // epistasis: 0 = the packed kernels' limits hold (16 folds, 16-bit counts per group / class); 1 = layouts and launches past them go through the
                               // wide listed-combination kernel (k_epi_combs_wide: 32-bit counts, up to EPI_WIDE_MAX_FOLDS folds); 2 = every listed-combination launch does
    long epi_triples_1pass = 1; // epistasis triple ranking with at most 10 folds: 1 = the 27 cells nine at a time (three walks, three waves per SIMD); 0 = the two-pass kernel; 2 (ablation build) = one pass with all counts in one lane
    long scan_lds = 0;         // bytes of (unused) LDS per workgroup of the stats / tdt scans: caps the waves in flight per CU
    long fisher_width = 16;    // lanes per variant in the Fisher p-pass (64, 32, 16 or 8): 64 / width variants per wave
    long inflate_wave = 1;     // bgzip decoder: 2 = one wave per block (hpgv_inflate2_kernels.h), 0 = one lane per block, 1 = by the number of blocks
    long tokenizer_tiles = 1;  // VCF text tokenizer: 1 = tile-parallel, two sweeps (count, scan, parse: the fastest); 2 = ONE sweep, the segments' states by look-back (k_tok_parse3: reads the text once, a third slower); 0 = count / mark / parse per line
    long batch_copy = 0;       // per-batch host entry points: 1 = copy page-locked rows to the device first (copy engine) instead of reading them in place
    long batch_fused = 1;      // per-batch host entry points: one fused kernel per call (0: copy + layout + scan + statistics kernels)
    long batch_lds_max = 65536;   // largest raw-row window the fused kernel stages in LDS (raised at hpgv_create when the device allows)
    // switches read ONCE from the environment at hpgv_create (include/hpgv.h "Environment"); no entry point reads the environment
    long stats_all2 = 1;       // HPGV_STATS_ALL2=0: every stats batch through the row-staging kernel (what shapes k_stats_all2 does not take use anyway)
    long assoc_rows = 1;       // HPGV_ASSOC_ROWS=0: text batches counted one workgroup per row (what wider cohorts fall back to)
    long pinned_noncoherent = 0;   // HPGV_PINNED_NONCOHERENT=1: page-locked buffers allocated non-coherent
    long vmm_trace = 0;        // HPGV_VMM_TRACE=1: hpgv_dev_commit narrates its mappings on stderr
    long decode_tiles = 1;     // HPGV_DECODE_TILES=0: windows of device-decoded text are tokenized with the counting sweep even when the decoder left its tile records
#ifdef HPGV_ABLATION
    long stats_rows = 0, stats_bs = 0, stats_debug = 0;      // HPGV_STATS_ROWS / _BS / _DEBUG: band length, workgroup size, chosen form of k_stats_all2
    long fisher_lds = 0;       // HPGV_FISHER_LDS: unused LDS bytes per workgroup of the Fisher pass
    long inflate_lds_pad = 0, inflate_wave_wgs = 0, inflate_lane_wgs = 0;      // HPGV_INFLATE_*: the decoder's occupancy experiments
#endif
    int n_cus = 256;
    // assoc
    Layout assoc;
    int nA = 0, nU = 0, chunksA = 0;
    DevBuf d_cond;                        // the condition of every column as given (padded with 2 to whole 16-byte chunks): k_assoc_rows' masks
    // label permutations of the association test (hpgv_set_perm_labels): one row per permutation in the assoc layout's column order
    // and pitch, zeros under the pads, perm_rows = n_perms rounded up to 16 rows; dropped by a new cohort
    DevBuf d_perm;
    int n_perms = 0, perm_rows = 0;
    // strata of the stratified association (hpgv_set_strata): the stratum image in the label matrix's format -- row 2k "stratum k and
    // affected", row 2k + 1 "stratum k and unaffected", strata_rows = 2 n_strata rounded up to 16 rows; dropped by a new cohort
    DevBuf d_strata;
    int n_strata = 0, strata_rows = 0;
    // ... and, for the permutation within strata (k_assoc_cmh_perm), the 64-column k-steps of the assoc layout that hold a member of
    // each stratum: CSR int32, n_strata + 1 offsets, then the ascending steps of stratum 0, 1, ..
    DevBuf d_strata_steps;
    DevBuf d_cmh_tables;                  // hpgv_assoc_cmh_dev's tables when the caller gives no buffer (the synchronous calls keep theirs in their slot)
    // covariates of the logistic regression (hpgv_set_covariates): one row of assoc.pitch doubles per covariate in the assoc layout's
    // column order, zeros under the pads; dropped by a new cohort
    DevBuf d_cov;
    int n_covar = 0;
    // the linear regression's model (hpgv_set_phenotype): the trait per VCF column and a host copy of the covariates, kept so that
    // either set call can rebuild the device image d_lin (hpgv_linear_kernels.h "LinArgs"); dropped by a new cohort
    std::vector<double> lin_y, lin_cov;
    bool has_pheno = false;
    DevBuf d_lin;
    // permutations of the linear statistic (hpgv_set_linear_perms): the image of hpgv_linear_perm_kernels.h -- tile 0 with Q and e, a
    // tile per 16 permutations -- and the 1 + n_linperms ss values behind it; dropped by a new cohort, phenotype or covariates
    DevBuf d_linperm;
    int n_linperms = 0;
    DevBuf d_linperm_rows;                // hpgv_assoc_linear_perm_dev's {mu, D} per row (the synchronous calls keep theirs in their slot)
    // tdt
    Layout tdt;
    hpgv::TdtPlan tdt_plan;
    // family flips of the TDT (hpgv_set_tdt_flips): one row of i8 signs per permutation in K order (the fast trios in plane order,
    // then the slow families, each part padded to whole 16-byte chunks: flip_pitch bytes), zeros under the pads, flip_rows = n_flips
    // rounded up to 16 rows; dropped by a new hpgv_set_families
    DevBuf d_flips;
    int n_flips = 0, flip_rows = 0, flip_pitch = 0;
    int tdt_families = 0;                 // n_families of hpgv_set_families: the length of a caller's flip row
    DevBuf d_flip_tail;                   // hpgv_tdt_perm_dev's slow-family differences per row (the synchronous calls keep theirs in their slot)
    // stats
    Layout stats;
    Layout sgroups;                       // [group 0 | pad16 | group 1 | ...]
    std::vector<uint32_t> sg_off;         // byte offset of every group's segment in the row
    std::vector<int> sg_size;             // samples per group
    DevBuf d_sg_chunks;                   // int32: first 16-byte chunk and chunk count of every group ([2 * n_groups])
    DevBuf d_group_of_col;                // uint8: group id of every column (0xFF: in no group), padded to whole 16-byte chunks -- k_stats_all2's masks
    bool all_grouped = false;             // every column is in a group: the last group's counters are "all minus the others"
    // mendelian errors
    Layout mendel;
    int mendel_trios = 0, mendel_pchunks = 0;
    hpgv::MendelLuts mendel_luts{};
    uint8_t *d_mendel_male = nullptr;
    // fisher
    double *d_lf = nullptr;
    double *d_lf_base = nullptr;       // the allocation: d_lf - 2 (padding for the two-entries-per-load reads of the Fisher pass)
    size_t n_lf = 0;
    size_t cap_lf = 0;                 // doubles behind d_lf (kept across tables: hipFree waits for the whole device)
    // synth scratch
    DevBuf d_thr;                         // uint32
    // profiling
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool have_scan_ev = false, have_stats_ev = false;
    std::vector<Slot *> slots;
    uint32_t *d_sink = nullptr;
    uint32_t *d_crc_tab = nullptr;     // tables of the BGZF CRC-32 check (hpgv_crc_kernels.h), built at first use
    // tokenizer scratch (newline counts per 4 KiB tile, line offsets), one set per stream that has
    // tokenized: calls on one stream are ordered by the stream, calls on different streams run
    // concurrently on the device and must not share it.  The table is guarded by tok_mu.
    struct TokScratch {
        hipStream_t stream = nullptr;
        DevBuf blocks, line_off, extra;
    };
    std::mutex tok_mu;
    std::vector<TokScratch *> tok_scratch;
    // address ranges whose backing grows (hpgv_dev_reserve / hpgv_dev_commit), under mu
    struct GrowRange { char *base = nullptr; size_t reserved = 0, committed = 0; std::vector<hipMemGenericAllocationHandle_t> pieces; std::vector<size_t> sizes; };
    std::vector<GrowRange> grow;
    // record filters of the text entry points (hpgv_set_text_filters); negative = off
    double filt_min_maf = -1.0, filt_max_missing = -1.0;
    long filt_max_mendel = -1;
    double filt_min_dom = -1.0, filt_min_rec = -1.0;   // hpgv_set_text_inheritance_filters
    // epistasis (calls are serialised by epi_mu)
    std::mutex epi_mu;
    EpiState epi;
};

namespace {

[[maybe_unused]] int fail(const hpgv_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) {
        ctx->err = buf;
        if (ctx->parent) {
            std::lock_guard<std::mutex> lk(ctx->parent->mu);
            ctx->parent->err = buf;
        }
    } else g_create_error = buf;
    return code;
}

// the C ABI never lets a C++ exception out: a failed host allocation inside an entry point (std::vector, std::string)
// becomes HPGV_ERR_NOMEM.  The slot lease and the device guard are released by their destructors during unwinding.
#define HPGV_ABI_TRY try {
#define HPGV_ABI_CATCH(ctx)                                                                         \
    } catch (const std::bad_alloc &) { return fail(ctx, HPGV_ERR_NOMEM, "out of host memory"); }     \
      catch (...) { return fail(ctx, HPGV_ERR_INVALID, "unexpected C++ exception inside the engine"); }

// group dispatch
inline bool is_group(const hpgv_ctx *c) { return c && !c->members.empty(); }
inline hpgv_ctx *first_member(hpgv_ctx *c) { return is_group(c) ? c->members[0] : c; }
inline const hpgv_ctx *first_member(const hpgv_ctx *c) { return is_group(c) ? c->members[0] : c; }
// the member a synchronous per-batch call runs on: fewest calls in flight, round-robin among equals
struct Dealt {
    hpgv_ctx *m;
    explicit Dealt(hpgv_ctx *g) {
        const unsigned n = (unsigned)g->members.size(), start = g->deal_next.fetch_add(1u, std::memory_order_relaxed) % n;
        m = g->members[start];
        int best = m->in_flight.load(std::memory_order_relaxed);
        for (unsigned k = 1; k < n && best > 0; ++k) {
            hpgv_ctx *c = g->members[(start + k) % n];
            const int f = c->in_flight.load(std::memory_order_relaxed);
            if (f < best) { best = f; m = c; }
        }
        m->in_flight.fetch_add(1, std::memory_order_relaxed);
    }
    ~Dealt() { m->in_flight.fetch_sub(1, std::memory_order_relaxed); }
};
#define GROUP_ALL(ctx, CALL)                                                                \
    if (is_group(ctx)) {                                                                    \
        for (hpgv_ctx *m_ : (ctx)->members) { const int rc_ = CALL; if (rc_) return rc_; }  \
        return HPGV_OK;                                                                     \
    }
#define GROUP_DEAL(ctx, CALL)                                                               \
    if (is_group(ctx)) { Dealt d_(ctx); hpgv_ctx *m_ = d_.m; return CALL; }
// a *_text call goes to the member on whose device the text already lies (hpgv_text_alias), else it is dealt
#define GROUP_DEAL_TEXT(ctx, text, CALL)                                                    \
    if (is_group(ctx)) {                                                                    \
        if (hpgv_ctx *m_ = alias_owner(ctx, text)) return CALL;                             \
        Dealt d_(ctx); hpgv_ctx *m_ = d_.m; return CALL;                                    \
    }

#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(ctx, HPGV_ERR_HIP, "%s failed: %s (%s:%d)", #call,                  \
                        hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

// makes ctx->device current for the scope of one API call
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            changed = (hipSetDevice(dev) == hipSuccess);
        }
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

[[maybe_unused]] constexpr size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// pitch of the VCF-order matrix the tokenizer writes for the *_text entry points
[[maybe_unused]] size_t raw_pitch_of(int n_samples) { return n_samples > 0 ? round_up((size_t)n_samples, 16) : 16; }

[[maybe_unused]] int upload_layout(hpgv_ctx *ctx, Layout &L) {
    // the table is kept when it is large enough: hipFree waits for every stream of the device, and a file run sets its
    // cohort while the decoder of the bgzip text is busy on streams of its own
    const size_t need = L.col_of_pos.size() * sizeof(int32_t);
    HIPCHK(ctx, L.d_cols.reserve(need));
    HIPCHK(ctx, hipMemcpy(L.d_cols.p, L.col_of_pos.data(), need, hipMemcpyHostToDevice));
    L.chunks = (int)(L.pitch / 16);
    L.set = true;
    return HPGV_OK;
}

// packed per-lane 16-bit partial sums bound the row length (hpgv_kernels.h)
constexpr int kScanUnroll = 8;       // unroll of the tdt/stats scans
constexpr int kMaxUnroll = 16;       // largest assoc unroll option
[[maybe_unused]] bool pitch_supported(size_t pitch) { return pitch / 16 / 64 + kMaxUnroll + 1 <= 2047; }

[[maybe_unused]] int acquire_slot(hpgv_ctx *ctx, Slot **out) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (Slot *s : ctx->slots)
        if (!s->busy) { s->busy = true; *out = s; return HPGV_OK; }
    Slot *s = new (std::nothrow) Slot();
    if (!s) return fail(ctx, HPGV_ERR_NOMEM, "out of host memory");
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete s; return fail(ctx, HPGV_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    s->busy = true;
    ctx->slots.push_back(s);
    *out = s;
    return HPGV_OK;
}
[[maybe_unused]] void release_slot(hpgv_ctx *ctx, Slot *s) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    s->busy = false;
}
struct SlotLease {
    hpgv_ctx *ctx; Slot *s = nullptr;
    explicit SlotLease(hpgv_ctx *c) : ctx(c) {}
    // an early return on a failure may leave copies into the caller's (or this call's stack) memory queued on the slot's
    // stream: they are waited for before the slot -- and the caller's buffers -- are handed back
    ~SlotLease() {
        if (!s) return;
        if (s->stream && hipStreamQuery(s->stream) == hipErrorNotReady) (void)hipStreamSynchronize(s->stream);
        (void)hipGetLastError();
        release_slot(ctx, s);
    }
};

// the opening of a synchronous entry point once its arguments are checked: the device current, a slot `s` leased until
// the call returns, `rc` for what follows
#define HPGV_LEASE_SLOT(ctx)                  \
    DeviceGuard g(ctx->device);               \
    SlotLease lease(ctx);                     \
    int rc = acquire_slot(ctx, &lease.s);     \
    if (rc) return rc;                        \
    Slot *s = lease.s;

template <typename F>
[[maybe_unused]] int launch_profiled(hpgv_ctx *ctx, hipStream_t st, int which /*0 scan,1 stats*/, F &&launch) {
    if (ctx->profile) HIPCHK(ctx, hipEventRecord(ctx->ev[2 * which], st));
    launch();
    HIPCHK(ctx, hipGetLastError());
    if (ctx->profile) {
        HIPCHK(ctx, hipEventRecord(ctx->ev[2 * which + 1], st));
        (which == 0 ? ctx->have_scan_ev : ctx->have_stats_ev) = true;
    }
    return HPGV_OK;
}

// Fisher's exact test needs the log-factorial table, long enough for the cohort's allele count
[[maybe_unused]] int logfact_check(const hpgv_ctx *ctx) {
    if (!ctx->d_lf) return fail(ctx, HPGV_ERR_STATE, "hpgv_set_logfact has not been called");
    if (ctx->assoc.set && ctx->n_lf < (size_t)2 * (ctx->nA + ctx->nU) + 1)
        return fail(ctx, HPGV_ERR_STATE, "log-factorial table has %zu entries, need %d", ctx->n_lf, 2 * (ctx->nA + ctx->nU) + 1);
    return HPGV_OK;
}

// where the parts of Slot::perm lie in a call over n rows and n_perms permutations: n_ge per row at 0, the batch maxima per
// permutation at round_up(4 n, 16), the rows' skip bytes behind them, then -- TDT flips: tail_pitch bytes per row -- the slow
// families' i8 differences from the next multiple of 16 on (the linear permutations: 24 bytes per row there, {mu, D} of every row,
// then t_obs of every row)
struct PermPlan {
    int32_t *d_n_ge = nullptr;
    double *d_max = nullptr;
    uint8_t *d_skip = nullptr;         // null when every row takes part
    int8_t *d_tail = nullptr;
};
struct PermOffsets { size_t max, skip, tail; };
constexpr PermOffsets perm_offsets(size_t n, size_t n_perms) {
    const size_t off_max = round_up(n * sizeof(int32_t), 16), off_skip = off_max + n_perms * sizeof(double);
    return {off_max, off_skip, round_up(off_skip + n, 16)};
}
// the synchronous calls launch without the *_dev wrappers' alignment refusals: the kernels' 64-bit atomics on the maxima need 8
// bytes, their 16-byte loads of the tail 16, at any row count -- odd ones above all
constexpr bool perm_offsets_aligned(size_t n, size_t n_perms) {
    return perm_offsets(n, n_perms).max % 16 == 0 && perm_offsets(n, n_perms).tail % 16 == 0 && perm_offsets(n, n_perms).skip >= perm_offsets(n, n_perms).max &&
           perm_offsets(n, n_perms).max >= n * sizeof(int32_t);
}
static_assert(perm_offsets_aligned(0, 1) && perm_offsets_aligned(1, 1) && perm_offsets_aligned(3, 130) && perm_offsets_aligned(70, 130) &&
              perm_offsets_aligned(71, 129) && perm_offsets_aligned(65, 17), "the plan of Slot::perm keeps the maxima and the tail aligned");

// room in the slot, the four parts placed, and the skip bytes (host, may be null) on their way to theirs
[[maybe_unused]] int perm_plan(hpgv_ctx *ctx, Slot *s, size_t n, size_t n_perms, const uint8_t *skip, size_t tail_pitch, PermPlan *P) {
    const PermOffsets off = perm_offsets(n, n_perms);
    HIPCHK(ctx, s->perm.reserve_slack(off.tail + n * tail_pitch + 16));
    char *base = s->perm.as<char>();
    P->d_n_ge = (int32_t *)base; P->d_max = (double *)(base + off.max); P->d_tail = (int8_t *)(base + off.tail);
    if (skip && n > 0) {
        P->d_skip = (uint8_t *)(base + off.skip);
        HIPCHK(ctx, hipMemcpyAsync(P->d_skip, skip, n, hipMemcpyHostToDevice, s->stream));
    }
    return HPGV_OK;
}

// the back half of the regressions' batch and text entry points (hpgv_assoc_logistic*, hpgv_assoc_linear*): room in the slot for a
// 48-byte record per row and, with coef, 2 (n_covar + 2) doubles per row behind them; launch(ctx, d_laid, n, args..., d_out, d_coef,
// stream) queues the kernel; then the caller's arrays, copied and waited for
template <typename Rec, typename F, typename... Args>
[[maybe_unused]] int regression_finish(hpgv_ctx *ctx, Slot *s, const Staged &S, Rec *out, double *coef, F launch, Args... args) {
    static_assert(sizeof(Rec) == 48, "the records of include/hpgv.h");
    if (S.n == 0) return HPGV_OK;
    const size_t n = (size_t)S.n, coef_bytes = coef ? n * (size_t)(2 * (ctx->n_covar + 2)) * sizeof(double) : 0;
    HIPCHK(ctx, s->dbl.reserve_slack(n * sizeof(Rec) + coef_bytes + 16));
    Rec *d_out = s->dbl.template as<Rec>();
    double *d_coef = coef ? (double *)(d_out + n) : nullptr;
    if (const int rc = launch(ctx, S.d_laid, S.n, args..., d_out, d_coef, s->stream)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, n * sizeof(Rec), hipMemcpyDeviceToHost, s->stream));
    if (coef) HIPCHK(ctx, hipMemcpyAsync(coef, d_coef, coef_bytes, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    return HPGV_OK;
}

}  // namespace

// defined in hpgv_capi.hip: the text aliases of a context (hpgv_text_alias, hpgv_text_alias_tiles)
bool tiles_of_device_text(hpgv_ctx *ctx, const char *d_text, hpgv_ctx::TextTiles *out);
const char *text_on_device(hpgv_ctx *ctx, const char *host_text);
hpgv_ctx *alias_owner(hpgv_ctx *group, const char *host_text);    // the member of a group on whose device `host_text` lies, or nullptr
// defined in hpgv_tool_capi.hip: the largest raw-row window the one-pass kernels may stage in LDS on this device (hpgv_create)
long hpgv_batch_lds_optin(const hipDeviceProp_t &prop, long fallback);
// defined in hpgv_text_capi.hip: the shared front half of the *_text entry points (and of hpgv_filter_text): text -> device,
// tokenize, record filters, lay out
// hpgv_linear_capi.hip: the linear model's device image from ctx->lin_y and ctx->lin_cov (a no-op without a phenotype)
int linear_image_rebuild(hpgv_ctx *ctx);

int text_front(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const char *text, size_t text_bytes, int max_lines, int *n_lines,
               uint64_t *line_off, uint32_t *field_off, int32_t *status, Staged *S, bool final_layout = true);
// defined in hpgv_tool_capi.hip: its twin for a host batch that goes through the kernel chain -- rows, then is_x, copied to the slot,
// the rows laid out for `which`.  The one place that says how much of the caller's matrix a chain call reads:
// (n_variants - 1) * pitch + n_samples bytes, the last row need not be a whole pitch.  n_variants may be 0
int stage_chain(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const uint8_t *gt, size_t pitch, int n_variants, const uint8_t *is_x,
                Staged *S);
// what a text call whose kernels skip lines keeps on the host while it runs: the status of its own when the caller gave none, and
// one byte per line.  Declared BEFORE the lease: copies queued into it end with the lease
struct TextSkip {
    std::vector<int32_t> own_status;
    std::vector<uint8_t> skip;
    const uint8_t *bytes() const { return skip.empty() ? nullptr : skip.data(); }
};
// defined in hpgv_text_capi.hip: text_front with the final layout (without it for a caller whose kernels read the raw matrix:
// hpgv_ibs_text), then the synchronise, then K->skip: 1 for the lines that hpgv_assoc_text's callers drop -- not a record, or
// rejected by a record filter (max_lines > 0)
int text_front_skip(hpgv_ctx *ctx, Slot *s, int which, const Layout &L, const char *text, size_t text_bytes, int max_lines, int *n_lines,
                    uint64_t *line_off, uint32_t *field_off, int32_t *status, TextSkip *K, Staged *S, bool final_layout = true);
// defined in hpgv_tool_capi.hip: the laid-out path of hpgv_assoc and hpgv_tdt in two halves, so that the permutation calls
// (hpgv_perm_capi.hip) queue their kernels between them.  *_chain: room in the slot (tally, dbl), scan, statistics (n = 0: room
// only).  *_copy_out: the copies into the caller's arrays, queued -- the caller synchronises (n = 0: nothing)
struct ChainOut {
    int32_t *d_tally = nullptr;                                   // per row, assoc: {A1, A2, U1, U2}; tdt: {t1, t2}
    double *d_odds = nullptr, *d_chisq = nullptr, *d_p = nullptr;
};
int assoc_chain(hpgv_ctx *ctx, Slot *s, int task, const Staged &S, ChainOut *C);
int assoc_copy_out(hpgv_ctx *ctx, Slot *s, int task, const Staged &S, const ChainOut &C, int32_t *A1, int32_t *A2, int32_t *U1, int32_t *U2,
                   double *odds, double *chisq, double *p);
int tdt_chain(hpgv_ctx *ctx, Slot *s, const Staged &S, ChainOut *C);
// (tu: the interleaved counts on the host; tdt_split_counts once the caller has synchronised)
int tdt_copy_out(hpgv_ctx *ctx, Slot *s, const Staged &S, const ChainOut &C, std::vector<int32_t> *tu, double *odds, double *chisq, double *p);
void tdt_split_counts(const std::vector<int32_t> &tu, int32_t *t1, int32_t *t2);
// defined in hpgv_text_capi.hip: the back half of hpgv_assoc_select_text -- the candidate lines of a staged text (a record, not
// filtered, p <= p_max; p_i at d_p + i * p_stride) numbered into sel, their raw rows compacted on the device and copied to rows_out
int select_rows(hpgv_ctx *ctx, Slot *s, const Staged &S, int n_samples, const int32_t *status, const char *d_p, size_t p_stride, double p_max,
                int32_t *sel, uint8_t *rows_out, size_t rows_pitch, int rows_cap, int *n_sel);
// defined in hpgv_cols_capi.hip, shared by the IBS, GRM and score units: the checks of a device matrix whose COLUMNS are contracted;
// the grid of a launch over `work` units in row ranges of `rows` rows (hpgv_cols_kernels.h "Grid"; `what` names the units where
// the grid is refused); the launch of the class counts {n0, n1, n2, missing} per row
namespace hpgv { struct ColsGrid; }
int cols_matrix_check(const hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols);
int cols_grid_fill(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, long long work, int rows, const char *what,
                   hpgv::ColsGrid *G);
int cols_class_launch(hpgv_ctx *ctx, const uint8_t *d_gt, size_t pitch, int n_variants, int n_cols, const uint8_t *d_skip, int32_t *d_class4, hipStream_t st);
// The front of the synchronous calls' back halves (S.n > 0): the matrix of a staged call as the kernels over sample COLUMNS read
// it -- the raw matrix in a pitch they take -- the rows' skip bytes on the device, the class counts queued on the slot's stream.
// skip (host, may be null) is copied to the slot; x_too: the rows the tokenizer flagged as chromosome X are skipped as well;
// need_skip: the caller's kernels write skip bytes, so they exist even where none is set (else d_skip may be null)
struct ColsFront {
    const uint8_t *d_gt = nullptr;
    size_t pitch = 0;
    uint8_t *d_skip = nullptr;
    int32_t *d_class4 = nullptr;
};
int cols_front(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, bool need_skip, ColsFront *F);
// the whole back half: cols_front, the tool's launches body(F) on s->stream, the class counts to the caller's class4, the
// synchronise (S.n = 0: the synchronise alone)
int cols_back(hpgv_ctx *ctx, Slot *s, const Staged &S, const uint8_t *skip, bool x_too, bool need_skip, int32_t *class4, const std::function<int(const ColsFront &)> &body);

// defined in hpgv_statsall_capi.hip: k_stats_all2 on a batch (0 = launched, 1 = not a batch it takes: run k_stats_all)
namespace hpgv { struct StatsAllArgs; }
int hpgv_launch_stats_all2(hpgv_ctx *ctx, hpgv::StatsAllArgs &A, DevBuf &row_cnt, hipStream_t st);
// k_assoc_rows: the allele counts from the tokenizer's raw rows (0 = launched, 1 = not a batch it takes: run k_batch)
int hpgv_launch_assoc_rows(hpgv_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int n_variants, const uint8_t *d_is_x, int32_t *d_counts, hipStream_t st);
// defined in hpgv_epi_capi.hip
void hpgv_epi_release(EpiState &E);
// defined in hpgv_epi_generic_capi.hip: in-fold counts of listed combinations of order 2 .. 5, device to device (the caller holds epi_mu)
int hpgv_epi_generic_counts(hpgv_ctx *ctx, int order, const int32_t *d_combs, int n_combs, int32_t *d_out);
// defined in hpgv_inflate_capi.hip: the CRC-32 tables of hpgv_crc_kernels.h in ctx->d_crc_tab, built at first use
int hpgv_crc_tables(hpgv_ctx *ctx);
// defined in hpgv_deflate_capi.hip: the launches of hpgv_bgzf_deflate_dev on `st` (the arguments checked, the device current)
int hpgv_bgzf_deflate_launch(hpgv_ctx *ctx, const char *d_text, const unsigned long long *d_seg_off, int n_segs, uint8_t *d_out,
                             unsigned long long *d_seg_out_off, void *d_scratch, hipStream_t st);
// defined in hpgv_group_capi.hip: streams, scratch and communicator of a group context (before its members go)
void hpgv_group_release(hpgv_ctx *group);
