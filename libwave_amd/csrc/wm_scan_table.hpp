// wm_scan_table.hpp -- the first half of the front of a call over a queue of scans: the scan table, the host clouds'
// upload and the pack into "batch positions" (the scans' points one after the other, scan-major), with each scan's box
// and finite count.  wm_scan_batch.hpp builds the scans' lattices on top of it (wm_cluster_extract_batch,
// wm_outlier_filter_batch); wm_sac_segment_batch needs no lattice and stops here.
//
// Included by the units that run a batch (each gets kernels of its own: the names are the cluster extraction's, where
// they were written).  Their single calls run the same kernels without a table: tab == nullptr and one ClScan by value
// (OlScans in wm_outlier.hip, SacScans in wm_sac.hip), which cl_find's look-up in a table of one never reads.
#pragma once
#include <string.h>

#include "wm_internal.hpp"
#include "wm_stage.hpp"

namespace wm {

namespace {

struct ClScan {  // one scan of a batch
    const unsigned char *raw;  // its records (device memory)
    unsigned n, off;           // points; its first batch position
    unsigned blk0;             // its first workgroup of the kernels over batch positions (kBlock points each)
    unsigned nf, g0;           // finite points; its first grid position
    unsigned lblk0;            // its first search workgroup (k_cluster_link, the outlier searches)
    unsigned aux0;             // the caller's own (the outlier filter: its first row of the moment sums)
    unsigned searched;         // its points that get a search lane: nf, or 0 where the caller wants no search
    unsigned long long cell0;  // its first cell
    GridDev g;                 // its lattice: cell_start = the scan's first cell, pts = the batch's cell-sorted array
};

// The last scan whose `field` is at or below x.  Scans without points (or without finite points, or without
// workgroups) share their value with the scan behind them, so the last one found is the one that owns x.
template <class Row, class Field>
__device__ __forceinline__ unsigned cl_find(const Row *__restrict__ tab, unsigned S, unsigned x, Field field) {
    unsigned k = 0, hi = S;
    while (hi - k > 1u) {
        const unsigned mid = (k + hi) >> 1;
        if (field(tab[mid]) <= x) k = mid;
        else hi = mid;
    }
    return k;
}
__device__ __forceinline__ unsigned cl_by_block(const ClScan *tab, unsigned S, unsigned b) {
    return cl_find(tab, S, b, [](const ClScan &s) { return s.blk0; });
}
__device__ __forceinline__ unsigned cl_by_point(const ClScan *tab, unsigned S, unsigned p) {
    return cl_find(tab, S, p, [](const ClScan &s) { return s.off; });
}

// float -> unsigned whose unsigned order is the float order (-0.0 canonicalised to +0.0 first)
__device__ __forceinline__ unsigned cl_orderable(float z) {
    const unsigned b = __float_as_uint(z == 0.f ? 0.f : z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Record j of an array of point records of out_stride bytes (a multiple of 4, at least 12): v's x y z as the packed
// cloud holds them, the bytes behind z zero.
__device__ __forceinline__ void cl_write_record(unsigned char *pout, size_t j, size_t out_stride, const float4 &v) {
    unsigned *o = reinterpret_cast<unsigned *>(pout + j * out_stride);
    o[0] = __float_as_uint(v.x);
    o[1] = __float_as_uint(v.y);
    o[2] = __float_as_uint(v.z);
    for (size_t w = 3; w < out_stride / 4; ++w) o[w] = 0u;
}

// ------------------------------------------------------------------ pack, boxes, finite counts
// k_pack's conversion into batch positions (.w = the batch position: the scan and the caller's index are recovered
// from it by the table), and per scan the box and the finite count -- bb: [3 S] minima, [3 S] maxima (orderable),
// [S] counts.  Minima, maxima and integer sums: the order of the atomics does not matter.
__global__ void __launch_bounds__(kBlock)
    k_cluster_pack(const ClScan *__restrict__ tab, unsigned S, size_t stride, float4 *__restrict__ out, unsigned *bb) {
    __shared__ unsigned s_lo[kBlock / 64][3], s_hi[kBlock / 64][3], s_cnt[kBlock / 64];
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, cnt = 0u;
    if (i < me.n) {
        const float *q = reinterpret_cast<const float *>(me.raw + (size_t) i * stride);
        float x = q[0], y = q[1], z = q[2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            lo[0] = hi[0] = cl_orderable(x);
            lo[1] = hi[1] = cl_orderable(y);
            lo[2] = hi[2] = cl_orderable(z);
            cnt = 1u;
        } else {
            x = y = z = __builtin_nanf("");
        }
        out[me.off + i] = make_float4(x, y, z, __uint_as_float(me.off + i));
    }
    for (int off = 32; off > 0; off >>= 1) {
        for (int d = 0; d < 3; ++d) {
            lo[d] = min(lo[d], (unsigned) __shfl_down(lo[d], off));
            hi[d] = max(hi[d], (unsigned) __shfl_down(hi[d], off));
        }
        cnt += __shfl_down(cnt, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int d = 0; d < 3; ++d) {
            s_lo[wave][d] = lo[d];
            s_hi[wave][d] = hi[d];
        }
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            for (int d = 0; d < 3; ++d) {
                lo[d] = min(lo[d], s_lo[w][d]);
                hi[d] = max(hi[d], s_hi[w][d]);
            }
            cnt += s_cnt[w];
        }
        if (cnt) {
            for (int d = 0; d < 3; ++d) {
                atomicMin(&bb[3u * k + d], lo[d]);
                atomicMax(&bb[3u * S + 3u * k + d], hi[d]);
            }
            atomicAdd(&bb[6u * S + k], cnt);
        }
    }
}

// What scan_table_pack hands on.
struct ScanTable {
    ClScan *tab = nullptr;          // the host mirror (pinned; valid until the stage's next batch)
    const ClScan *d_tab = nullptr;  // the device table
    unsigned S = 0;
    size_t total = 0, blocks = 0;   // batch positions and their workgroups of kBlock
    size_t table_bytes = 0;
};

// On the context's stream: the table's first half (raw, n, off, blk0) and the host clouds up (PairStage),
// k_cluster_pack into `pts` (grown to the batch's points), the boxes and the finite counts into `bb` (grown to
// bb_bytes >= 7 S words; the bytes behind the minima are zeroed).  `scans`: the caller's {pts, n} rows, checked by the
// caller (no null cloud with points, the points in all below 2^31).  ev_a is recorded behind the upload
// (PairStage::submit).  Nothing is fetched and nothing waited for: bb's fetch is the caller's.
template <class Scan>
int scan_table_pack(wm_ctx *ctx, PairStage &stg, const Scan *scans, unsigned S, size_t stride, int mem, DevBuf &pts,
                    DevBuf &bb_buf, size_t bb_bytes, ScanTable *out) {
    hipStream_t st = ctx->stream;
    size_t total = 0, cloud_bytes = 0, blocks = 0;
    for (unsigned k = 0; k < S; ++k) {
        total += scans[k].n;
        cloud_bytes += align_up256(scans[k].n * stride);
        blocks += (scans[k].n + kBlock - 1) / kBlock;
    }
    const size_t table_bytes = align_up256((size_t) S * sizeof(ClScan));
    WM_TRY(stg.begin(ctx, table_bytes, cloud_bytes, 0, 0, mem));
    ClScan *tab = stg.table<ClScan>();
    unsigned off = 0, blk = 0;
    for (unsigned k = 0; k < S; ++k) {
        ClScan &t = tab[k];
        t = ClScan{};
        t.n = (unsigned) scans[k].n;
        t.off = off;
        t.blk0 = blk;
        WM_TRY(stg.up.add(ctx, scans[k].pts, scans[k].n * stride, &t.raw));
        off += t.n;
        blk += (t.n + kBlock - 1) / kBlock;
    }
    const ClScan *d_tab = stg.d_table<ClScan>();
    WM_HIP(ctx, pts.reserve(total * sizeof(float4)));
    WM_HIP(ctx, bb_buf.reserve(bb_bytes));
    unsigned *bb = bb_buf.as<unsigned>();
    WM_TRY(stg.submit(ctx));
    WM_HIP(ctx, hipMemsetAsync(bb, 0xFF, (size_t) S * 3 * 4, st));
    WM_HIP(ctx, hipMemsetAsync(bb + 3 * (size_t) S, 0, bb_bytes - (size_t) S * 3 * 4, st));
    if (blocks) hipLaunchKernelGGL(k_cluster_pack, dim3((unsigned) blocks), dim3(kBlock), 0, st, d_tab, S, stride, pts.as<float4>(), bb);
    WM_HIP(ctx, hipGetLastError());
    out->tab = tab;
    out->d_tab = d_tab;
    out->S = S;
    out->total = total;
    out->blocks = blocks;
    out->table_bytes = table_bytes;
    return WM_OK;
}

}  // namespace

}  // namespace wm
