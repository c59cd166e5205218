// hpgv_deflate_capi.hip -- C ABI of the BGZF compressor (include/hpgv.h): device text and segment bounds -> whole BGZF
// members (hpgv_bgzf_deflate_dev), and the same on host buffers (hpgv_bgzf_compress).  The partition / multisplit twins that
// deflate their parts are in hpgv_lines_capi.hip, beside the plain ones whose front half they share.
#include "hpgv_internal.h"
#include "hpgv_deflate_kernels.h"

static_assert(HPGV_BGZF_BLOCK_TEXT == hpgv::DFL_BLOCK, "block size of the header and of the kernel");

// blocks that text_bytes of text in n_segs segments can make, at most
static size_t dfl_max_blocks(uint64_t text_bytes, int n_segs) { return (size_t)(text_bytes / hpgv::DFL_BLOCK) + (size_t)(n_segs > 0 ? n_segs : 0); }

int hpgv_bgzf_deflate_launch(hpgv_ctx *ctx, const char *d_text, const unsigned long long *d_seg_off, int n_segs, uint8_t *d_out,
                             unsigned long long *d_seg_out_off, void *d_scratch, hipStream_t st) {
    if (n_segs == 0) {
        HIPCHK(ctx, hipMemsetAsync(d_seg_out_off, 0, sizeof(unsigned long long), st));
        return HPGV_OK;
    }
    if (const int rc = hpgv_crc_tables(ctx)) return rc;
    const int hb = (n_segs + 1023) / 1024;
    unsigned long long *seg_blk = (unsigned long long *)d_scratch, *block = seg_blk + (size_t)n_segs + 1;
    hipLaunchKernelGGL(hpgv::k_dfl_seg_sums, dim3((unsigned)hb), dim3(1024), 0, st, d_seg_off, n_segs, block);
    hipLaunchKernelGGL(hpgv::k_head_bases, dim3(1), dim3(1024), 0, st, block, hb);
    hipLaunchKernelGGL(hpgv::k_dfl_seg_offsets, dim3((unsigned)hb), dim3(1024), 0, st, d_seg_off, n_segs, (const unsigned long long *)block, seg_blk);
    // the number of blocks is on the device: single waves stride over them, 16 per CU (a wave beyond the last block ends at once)
    const unsigned cus = (unsigned)(ctx->n_cus > 0 ? ctx->n_cus : 256);
    hipLaunchKernelGGL(hpgv::k_bgzf_deflate, dim3(16 * cus), dim3(64), 0, st, (const uint8_t *)d_text, d_seg_off, n_segs, d_scratch,
                       (const uint32_t *)ctx->d_crc_tab);
    hipLaunchKernelGGL(hpgv::k_dfl_member_offsets, dim3(1), dim3(1024), 0, st, d_scratch, n_segs);
    hipLaunchKernelGGL(hpgv::k_dfl_copy, dim3(4 * cus), dim3(256), 0, st, d_scratch, n_segs, d_out, d_seg_out_off);
    HIPCHK(ctx, hipGetLastError());
    return HPGV_OK;
}

extern "C" {

size_t hpgv_bgzf_deflate_bound(uint64_t text_bytes, int n_segs) {
    return (size_t)text_bytes + dfl_max_blocks(text_bytes, n_segs) * hpgv::DFL_OVERHEAD;
}

size_t hpgv_bgzf_deflate_scratch_bytes(uint64_t text_bytes, int n_segs) {
    if (n_segs <= 0) return 0;
    const size_t nb = dfl_max_blocks(text_bytes, n_segs);
    return hpgv::dfl_head_bytes(n_segs) + hpgv::dfl_meta_bytes(nb) + nb * hpgv::DFL_SLOT;
}

int hpgv_bgzf_deflate_dev(hpgv_ctx *ctx, const char *d_text, const uint64_t *d_seg_off, int n_segs, uint8_t *d_out,
                          uint64_t *d_seg_out_off, void *d_scratch, void *stream) {
    HPGV_ABI_TRY
    ctx = first_member(ctx);
    if (!ctx) return HPGV_ERR_INVALID;
    if (n_segs < 0 || !d_seg_out_off || (n_segs > 0 && (!d_text || !d_seg_off || !d_out || !d_scratch || ((uintptr_t)d_scratch & 15))))
        return fail(ctx, HPGV_ERR_INVALID, "bad bgzf_deflate_dev arguments");
    DeviceGuard g(ctx->device);
    return hpgv_bgzf_deflate_launch(ctx, d_text, (const unsigned long long *)d_seg_off, n_segs, d_out, (unsigned long long *)d_seg_out_off,
                                    d_scratch, (hipStream_t)stream);
    HPGV_ABI_CATCH(ctx)
}

int hpgv_bgzf_compress(hpgv_ctx *ctx, const char *text, size_t text_bytes, uint8_t *out, size_t out_cap, size_t *out_bytes) {
    HPGV_ABI_TRY
    GROUP_DEAL(ctx, hpgv_bgzf_compress(m_, text, text_bytes, out, out_cap, out_bytes))
    if (!ctx) return HPGV_ERR_INVALID;
    if (!out_bytes || (text_bytes > 0 && !text)) return fail(ctx, HPGV_ERR_INVALID, "bad bgzf_compress arguments");
    *out_bytes = 0;
    if (text_bytes == 0) return HPGV_OK;
    HPGV_LEASE_SLOT(ctx)
    const size_t scratch = hpgv_bgzf_deflate_scratch_bytes(text_bytes, 1), bound = hpgv_bgzf_deflate_bound(text_bytes, 1);
    HIPCHK(ctx, s->text.reserve_slack(text_bytes + 16));
    HIPCHK(ctx, s->members.reserve_slack(bound + 16));
    HIPCHK(ctx, s->dfl.reserve_slack(scratch + 64));
    unsigned long long *d_seg = (unsigned long long *)(s->dfl.as<char>() + scratch);      // behind the kernels' scratch: seg_off[2], seg_out_off[2]
    const unsigned long long seg[2] = {0, (unsigned long long)text_bytes};
    unsigned long long got[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(s->text.p, text, text_bytes, hipMemcpyHostToDevice, s->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_seg, seg, sizeof seg, hipMemcpyHostToDevice, s->stream));
    if ((rc = hpgv_bgzf_deflate_launch(ctx, s->text.as<const char>(), d_seg, 1, s->members.as<uint8_t>(), d_seg + 2, s->dfl.p, s->stream))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(got, d_seg + 2, sizeof got, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    const size_t made = (size_t)got[1];
    if (!out || made > out_cap) return fail(ctx, HPGV_ERR_INVALID, "the members take %zu bytes, out has room for %zu", made, out_cap);
    HIPCHK(ctx, hipMemcpyAsync(out, s->members.p, made, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(ctx, hipStreamSynchronize(s->stream));
    *out_bytes = made;
    return HPGV_OK;
    HPGV_ABI_CATCH(ctx)
}

}  // extern "C"
