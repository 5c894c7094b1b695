// wm_stage.hpp -- how a batch of pairs gets to the device and its results back: the one staging
// sequence of wm_icp_batch_match, wm_gicp_batch_match, wm_ndt_batch_match, the batched voxel filter and
// wm_ground_segment_batch (whose table rows are scans, not pairs: the helper does not look into a row)
// (the structs: wm_internal.hpp, where the context holds them).  On the context's stream, in this order:
// the host clouds in slices, the table, ev_a, the caller's kernels, ev_b, the outputs.
#pragma once
#include <string.h>

#include "wm_internal.hpp"

namespace wm {

inline int SliceUpload::begin(wm_ctx *ctx, size_t head, size_t cloud_bytes, int mem) {
    host_clouds = mem == WM_MEM_HOST;
    const size_t bytes = head + (host_clouds ? cloud_bytes : 0);
    WM_HIP(ctx, dev.reserve(bytes));
    WM_HIP(ctx, host.reserve(bytes));
    off = sent = head;
    return WM_OK;
}

inline int SliceUpload::add(wm_ctx *ctx, const void *pts, size_t bytes, const unsigned char **on_device) {
    if (!host_clouds) {
        *on_device = static_cast<const unsigned char *>(pts);
        return WM_OK;
    }
    if (bytes) memcpy(host.as<unsigned char>() + off, pts, bytes);
    *on_device = dev.as<unsigned char>() + off;
    off += align_up256(bytes);
    return off - sent >= ((size_t) 2 << 20) ? flush(ctx) : WM_OK;
}

inline int SliceUpload::flush(wm_ctx *ctx) {
    if (off > sent)
        WM_HIP(ctx, hipMemcpyAsync(dev.as<unsigned char>() + sent, host.as<unsigned char>() + sent, off - sent, hipMemcpyHostToDevice, ctx->stream));
    sent = off;
    return WM_OK;
}

inline int PairStage::begin(wm_ctx *ctx, size_t table_bytes_, size_t cloud_bytes, size_t work_bytes, size_t out_bytes, int mem) {
    table_bytes = table_bytes_;
    WM_TRY(up.begin(ctx, table_bytes, cloud_bytes, mem));
    WM_HIP(ctx, d_work.reserve(work_bytes));
    WM_HIP(ctx, d_out.reserve(out_bytes));
    WM_HIP(ctx, h_out.reserve(out_bytes));
    work = Carver{d_work.as<unsigned char>(), 0};
    // the stream may still be reading the pinned mirror for the previous batch
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

inline int PairStage::submit(wm_ctx *ctx) {
    WM_TRY(up.flush(ctx));
    WM_HIP(ctx, hipMemcpyAsync(up.dev.p, up.host.p, table_bytes, hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(ctx, hipEventRecord(ctx->ev_a, ctx->stream));
    return WM_OK;
}

inline int PairStage::collect(wm_ctx *ctx, size_t out_bytes, float *kernel_ms) {
    WM_HIP(ctx, hipGetLastError());  // (the caller's launches)
    WM_HIP(ctx, hipEventRecord(ctx->ev_b, ctx->stream));
    WM_HIP(ctx, hipMemcpyAsync(h_out.p, d_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    WM_TRY(sync_sleeping(ctx));  // (milliseconds: the registrations of the whole batch)
    if (kernel_ms) (void) hipEventElapsedTime(kernel_ms, ctx->ev_a, ctx->ev_b);
    return WM_OK;
}

}  // namespace wm
