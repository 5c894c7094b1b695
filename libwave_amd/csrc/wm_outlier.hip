// wm_outlier.hip -- outlier removal on the device: pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval as one
// cloud-in / indices-out call (wm_outlier_filter), shaped like wm_ground_segment: the call packs the cloud, builds a
// cell-sorted grid over it for this call alone, and works in a workspace of its own on the context.
// wm_outlier_filter_batch is the same for a queue of scans: ONE set of kernels with a scan dimension, as
// wm_ground_segment_batch and wm_cluster_extract_batch.
//
// The rules (written from PCL 1.8; PCL is not linked, the checker is tests/outlier_reference.py):
//   [PCL-upstream filters/impl/statistical_outlier_removal.hpp applyFilterIndices]  per point the mean_k + 1 nearest
//     points of the cloud, itself included; the first entry (d2 = 0: the point or a duplicate of it) is skipped, the
//     other mean_k distances sqrt((double) d2) are added in list order in double, and the point's mean distance is
//     (float) (sum / mean_k).  Over the n finite points, the float distances widened to double:
//       mean = sum d / n,  var = (sum d^2 - (sum d)^2 / n) / (n - 1),  stddev = sqrt(var),
//       threshold = mean + stddev_mult * stddev;  outlier iff (double) dist > threshold (a NaN threshold removes nothing).
//   [PCL-upstream filters/impl/radius_outlier_removal.hpp applyFilterIndices, FLANN RadiusResultSet]  r2 = (float)
//     (radius * radius), the product in double; a point's neighbours are the OTHER finite points with d2 < r2
//     (strict, as FLANN's radius set); inlier iff their number >= min_neighbors (PCL: "k <= min_pts is an outlier" with
//     the point itself in k).
//   Both: d2 is g_d2's float form, (dx * dx + dy * dy) + dz * dz with nothing fused; lists are ordered by
//     (d2, index); kept indices ascend; `negative` returns the outliers.
//   Deviation from PCL: a non-finite point is nobody's neighbour, enters no statistic, gets WM_OUTLIER_NONE and is
//     returned with neither setting of `negative` (PCL keeps it, with distance 0) -- as wm_set_source drops such points.
//
// The scans of a call reach the kernels as an OlScans: a table of ClScan rows in device memory (a batch), or
// tab == nullptr and the one scan by value in the kernel arguments (the single call: no table, no staging).  So every
// output of scan k of a batch EQUALS the single call's for that scan alone, bit for bit, because the same code made it.
//   front      the single call: pack_cloud, compute_bbox, build_call_grid.  A batch: wm_scan_batch.hpp's, shared with
//              wm_cluster_extract_batch -- batch positions (scan-major), a lattice per scan under the shared 2^26-cell
//              budget, ONE cell-sorted array.  Coarser cells change no output: the searches are exact whatever the lattice.
//   searches   k_outlier_mean_dist<K> (knn_search<K> straight into the mean distance: the lists never reach memory) or
//              k_outlier_radius<EXACT> (one lane per query over the rows of the box [q - r, q + r]).  A search workgroup
//              is one wave of 64 queries of ONE scan in grid order, found from the table of first workgroups, and uses
//              that scan's GridDev: a walk never meets a point of another scan.  .w is the batch position, monotonic in
//              the caller index inside a scan, so the (d2, index) tie order does not depend on what else is in the
//              batch.  A scan of a batch that is not converged (0 < n_finite < mean_k + 1) gets no search workgroup and
//              no row of the moment sums; its labels are NONE and nothing of it is kept.
//   moments    k_outlier_moments + k_outlier_threshold: the two sums in double, a fixed tree over the scan's points in
//              CALLER order (the cell sort's order inside a cell is the atomics' arrival order and must not reach a
//              sum) whose shape depends on that scan's n alone: rows = min(blocks_of(n), 1024) workgroups of 256 threads
//              (outlier_rows; a scan's first row is ClScan::aux0), thread t takes points t, t + rows * 256, ...; the
//              wave's shuffle tree; thread 0 over the four waves; one wave per scan over its rows.  No sum runs through
//              atomics over floats or doubles.
//   compaction k_outlier_label over batch positions with the scan's own threshold, ONE exclusive scan over the call (a
//              scan's offset is the scan's value at its first position), k_outlier_emit: the kept indices, local to
//              their scan and ascending, the scans' offsets and, if wanted, the points.
//   the end    mean, stddev, threshold per scan and the offsets behind them come back in one copy; launches and waits
//              do not depend on the number of scans.
#include "wm_radius_walk.hpp"
#include "wm_scan_batch.hpp"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

constexpr int kOutBlock = 64;        // queries (threads) of a search workgroup: one wave, as k_gicp_cov (see there)
constexpr int kMomBlocksMax = 1024;  // partial rows of the moment sums (their number depends on n alone)

// The scans of a call.  The single call fills `one` with n, nf, searched, its GridDev and zeros (it owns position,
// workgroup and row 0 of everything); a look-up in a table of one never reads the table (cl_find).  A batch sets of
// `one` only g.pts and g.cell_start: the arrays every scan's GridDev points into (ol_lane).
struct OlScans {
    const ClScan *tab;
    unsigned S;
    ClScan one;
    __device__ __forceinline__ ClScan scan(unsigned k) const {
        if (tab) return tab[k];
        return one;
    }
};

// Search workgroup blockIdx.x is one wave of 64 queries of ONE scan, whose lattice `g` it walks: queries in the grid's
// own (cell-sorted) order -- a wave's 64 queries scan the same few rows of cells.  Returns the lane's grid position;
// `end`: behind the scan's last searched one.  The scan's fields are taken into scalars here, once.
__device__ __forceinline__ unsigned ol_lane(const OlScans &sc, GridDev &g, unsigned &end) {
    const ClScan *__restrict__ tab = sc.tab;
    g = sc.one.g;
    unsigned g0 = 0u, lblk0 = 0u, searched = sc.one.searched;
    if (tab) {
        const unsigned k = cl_by_search(tab, sc.S, blockIdx.x);
        g = tab[k].g;
        g0 = tab[k].g0;
        lblk0 = tab[k].lblk0;
        searched = tab[k].searched;
        // The cell-sorted array and the lattices' cell_start are the call's own, whichever the scan: a batch has them
        // in `one` too, and the walk addresses them from there.  A pointer read from the table is a generic (flat)
        // address to the compiler -- flat_load: an LDS-aperture check, and lgkmcnt coupling with the walk's run lists
        // -- and ONE such source would make the single call's loads flat as well.
        g.pts = sc.one.g.pts;
        g.cell_start = sc.one.g.cell_start + tab[k].cell0;
    }
    end = g0 + searched;
    return g0 + (blockIdx.x - lblk0) * kOutBlock + threadIdx.x;
}

// ------------------------------------------------------------------ statistical: mean distance to the mean_k nearest
// The result is stored under the point's batch position (.w).  Only finite points are in the grid; k = mean_k + 1 <=
// their number in the scan.
template <int K>
__global__ void __launch_bounds__(kOutBlock) __attribute__((amdgpu_waves_per_eu(K <= 10 ? 6 : (K <= 12 ? 5 : 1))))
    k_outlier_mean_dist(OlScans sc, int k, float r0_cells, float *__restrict__ dist_out) {
    __shared__ uint2 s_runs[kKnnRows * kOutBlock];
    GridDev g;
    unsigned end;
    const unsigned i = ol_lane(sc, g, end);
    if (i >= end) return;
    const float4 q = g.pts[i];
    unsigned long long best[K];
    knn_search<K>(g, q.x, q.y, q.z, k, r0_cells, best, s_runs, threadIdx.x, kOutBlock);
    double s = 0.0;
#pragma unroll
    for (int j = 1; j < K; ++j)
        if (j < k) s += sqrt((double) __uint_as_float((unsigned) (best[j] >> 32)));
    dist_out[__float_as_uint(q.w)] = (float) (s / (double) (k - 1));
}

// the scan's rows of the moment sums: min(blocks_of(n), kMomBlocksMax) for a searched scan, else none
__host__ __device__ __forceinline__ unsigned outlier_rows(unsigned n, unsigned searched) {
    const unsigned b = (n + kBlock - 1) / kBlock;
    return searched ? (b < (unsigned) kMomBlocksMax ? b : (unsigned) kMomBlocksMax) : 0u;
}

// sum d and sum d^2 over the scan's finite points, caller order.  Workgroup blockIdx.x is row (blockIdx.x - aux0) of
// its scan's tree: thread t of the tree takes points t, t + T, ...; a wave's 64 sums by a shuffle tree, a workgroup's
// four by thread 0 in wave order -> row blockIdx.x of `part`
__global__ void __launch_bounds__(kBlock)
    k_outlier_moments(OlScans sc, const float4 *__restrict__ pts, const float *__restrict__ dist, double *__restrict__ part) {
    const ClScan me = sc.scan(cl_find(sc.tab, sc.S, blockIdx.x, [](const ClScan &s) { return s.aux0; }));
    const unsigned stride = outlier_rows(me.n, me.searched) * kBlock;
    double s1 = 0.0, s2 = 0.0;
    for (unsigned i = (blockIdx.x - me.aux0) * kBlock + threadIdx.x; i < me.n; i += stride) {
        const float x = pts[me.off + i].x;
        if (x == x) {
            const double d = (double) dist[me.off + i];
            s1 += d;
            s2 += d * d;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off);
        s2 += __shfl_down(s2, off);
    }
    __shared__ double l1[kBlock / 64], l2[kBlock / 64];
    if ((threadIdx.x & 63) == 0) {
        l1[threadIdx.x >> 6] = s1;
        l2[threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            s1 += l1[w];
            s2 += l2[w];
        }
        part[2 * (size_t) blockIdx.x] = s1;
        part[2 * (size_t) blockIdx.x + 1] = s2;
    }
}

// a scan's rows added in one fixed order (one wave per scan, blockIdx.x: lane l takes rows l, l + 64, ..., then the
// shuffle tree) -> res[4 k]: mean, stddev, threshold; a scan without rows (empty, nothing finite, not converged) keeps
// the zeros res was cleared to
__global__ void __launch_bounds__(64)
    k_outlier_threshold(OlScans sc, const double *__restrict__ part, double stddev_mult, double *__restrict__ res) {
    const ClScan me = sc.scan(blockIdx.x);
    const unsigned rows = outlier_rows(me.n, me.searched);
    if (!rows) return;
    part += 2 * (size_t) me.aux0;
    double s1 = 0.0, s2 = 0.0;
    for (unsigned r = threadIdx.x; r < rows; r += 64) {
        s1 += part[2 * r];
        s2 += part[2 * r + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off);
        s2 += __shfl_down(s2, off);
    }
    if (threadIdx.x == 0) {
        const double n_finite = (double) me.nf;
        const double mean = s1 / n_finite;
        const double var = (s2 - s1 * s1 / n_finite) / (n_finite - 1.0);
        const double sd = sqrt(var);
        res[4 * (size_t) blockIdx.x] = mean;
        res[4 * (size_t) blockIdx.x + 1] = sd;
        res[4 * (size_t) blockIdx.x + 2] = mean + stddev_mult * sd;
    }
}

// ------------------------------------------------------------------ radius: neighbours within r
// One lane per query (result under .w) over the rows of the box of cells covering [q - r, q + r]: radius_walk
// (wm_radius_walk.hpp, shared with k_cluster_link).  hits counts d2 < r2, the query itself among them (d2 = 0)
// whenever r2 > 0; the count written is the OTHER points'.
// EXACT: the count is exact.  Otherwise a lane stops once it has seen `stop` hits (min_neighbors + 1, itself
// included): what it writes then is >= min_neighbors, which is all the labelling asks.
template <bool EXACT>
__global__ void __launch_bounds__(kOutBlock)
    k_outlier_radius(OlScans sc, float r2, float rf, unsigned stop, int *__restrict__ count_out) {
    __shared__ uint2 s_runs[kKnnRows * kOutBlock];
    GridDev g;
    unsigned end;
    const unsigned i = ol_lane(sc, g, end);
    if (i >= end) return;
    const float4 q = g.pts[i];
    unsigned hits = 0;
    radius_walk<!EXACT>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kOutBlock, [&](unsigned, const float4 &t) {
        hits += g_d2(q.x, q.y, q.z, t) < r2 ? 1u : 0u;
        return !EXACT && hits >= stop;
    });
    const unsigned self = r2 > 0.f ? 1u : 0u;
    count_out[__float_as_uint(q.w)] = (int) (hits - (hits >= self ? self : 0u));
}

// ------------------------------------------------------------------ labels and the kept list (caller order)
// Over batch positions: a workgroup belongs to one scan and reads that scan's threshold (res[4 k + 2]; res == nullptr:
// the radius filter).  A scan with finite points that is not searched is not converged: NONE, not kept.
__global__ void __launch_bounds__(kBlock)
    k_outlier_label(OlScans sc, const float4 *__restrict__ pts, const float *__restrict__ dist, const double *__restrict__ res,
                    const int *__restrict__ counts, int min_neighbors, int negative, uint8_t *__restrict__ labels,
                    unsigned *__restrict__ keep) {
    const unsigned k = cl_by_block(sc.tab, sc.S, blockIdx.x);
    const ClScan me = sc.scan(k);
    const unsigned li = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    if (li >= me.n) return;
    const unsigned i = me.off + li;
    const float x = pts[i].x;
    const bool finite = x == x && me.searched != 0u;
    bool outlier = false;
    if (finite) outlier = res ? (double) dist[i] > res[4 * (size_t) k + 2] : counts[i] < min_neighbors;
    if (labels) labels[i] = finite ? (outlier ? WM_OUTLIER_OUTLIER : WM_OUTLIER_INLIER) : WM_OUTLIER_NONE;
    keep[i] = finite && outlier == (negative != 0) ? 1u : 0u;
}

// pos = the exclusive scan of keep over the call (total + 1 entries).  offs[k] = pos at scan k's first position,
// offs[S] = the number kept; a kept point: its index inside its scan and, for points_out, its record
// (cl_write_record: a kept point is finite, and a finite point is packed bit for bit).
__global__ void __launch_bounds__(kBlock)
    k_outlier_emit(OlScans sc, unsigned blocks, unsigned total, const float4 *__restrict__ pts, const unsigned *__restrict__ keep,
                   const unsigned *__restrict__ pos, int *__restrict__ out, size_t cap, unsigned char *__restrict__ pout,
                   size_t out_stride, unsigned *__restrict__ offs) {
    const size_t t = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (t <= sc.S) offs[t] = pos[t < sc.S ? sc.scan((unsigned) t).off : total];
    if (blockIdx.x >= blocks) return;
    const ClScan me = sc.scan(cl_by_block(sc.tab, sc.S, blockIdx.x));
    const unsigned li = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    if (li >= me.n) return;
    const unsigned i = me.off + li;
    if (!keep[i]) return;
    const unsigned j = pos[i];
    if (j >= cap) return;
    out[j] = (int) li;
    if (pout) cl_write_record(pout, j, out_stride, pts[i]);
}

__global__ void __launch_bounds__(kBlock) k_outlier_fill(int *__restrict__ p, unsigned n, int v) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

// The context's workspace of this filter: its own buffers, shared with nothing else on the context.
struct OutlierWs {
    DevBuf dist, counts, labels, keep, pos, part;
    DevBuf res;         // mean, stddev, threshold (and a spare) per scan, then the scans' offsets
    DevBuf out, pout;   // host outputs on their way
    ScanBatchBufs sb;   // the packed cloud and its grid; a batch's front (wm_scan_batch.hpp)
    PinnedBuf h_res;    // res on the host
};

void outlier_release(wm_ctx *ctx) {
    OutlierWs *w = static_cast<OutlierWs *>(ctx->outlier);
    if (!w) return;
    DevBuf *bufs[] = {&w->dist, &w->counts, &w->labels, &w->keep, &w->pos, &w->part, &w->res, &w->out, &w->pout};
    for (DevBuf *b : bufs) b->release();
    w->sb.release();
    w->h_res.release();
    delete w;
    ctx->outlier = nullptr;
}

namespace {

bool outlier_params_ok(const wm_outlier_params *p) {
    if (p->method == WM_OUTLIER_STATISTICAL) return p->mean_k >= 1 && p->mean_k <= 31;
    if (p->method == WM_OUTLIER_RADIUS) return std::isfinite(p->radius) && p->radius > 0 && p->min_neighbors >= 0;
    return false;
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

// no cell of the radius filter is smaller: its box [q - r, q + r] must span a bounded number of rows (DESIGN.md 4.8
// has the measurements)
float ol_floor_h(const wm_ctx *ctx, const wm_outlier_params *p) {
    return p->method == WM_OUTLIER_STATISTICAL ? 0.f : fminf((float) p->radius, 1.0e30f) / ctx->tune_outlier_cell_div;
}

// What the front of a call (one scan or a batch) hands to the kernels behind the grid, and where the results go.
struct OlCall {
    OlScans sc{nullptr, 1, ClScan{}};  // the device table, or the one scan
    const ClScan *h_tab = nullptr;     // a batch: the table's host mirror
    size_t n = 0;                      // the call's points (batch positions)
    unsigned blocks = 0, search_blocks = 0, rows = 0;  // their workgroups, the searches', the rows of the moment sums
    const wm_outlier_params *p = nullptr;
    bool host_out = true, timed = false;
    int32_t *indices_out = nullptr;
    size_t cap = 0;
    void *points_out = nullptr;
    size_t out_stride = 0;
    size_t *offsets_out = nullptr;  // S + 1
    uint8_t *labels_out = nullptr;
    float *mean_dist_out = nullptr;
    int32_t *counts_out = nullptr;
    const int *status = nullptr;  // a batch: a scan that is not WM_OK gets no statistics
    wm_outlier_stats *stats = nullptr;
    // the outputs' places on the device (ol_place)
    uint8_t *d_labels = nullptr;
    float *d_dist = nullptr;
    int *d_counts = nullptr, *d_out = nullptr;
    unsigned char *d_pout = nullptr;
    size_t d_cap = 0;
    float ms = 0.f;  // result: ev_a to behind the kept list

    bool stat() const { return p->method == WM_OUTLIER_STATISTICAL; }
    size_t res_bytes() const { return (size_t) sc.S * 4 * sizeof(double); }
    size_t fetch_bytes() const { return res_bytes() + ((size_t) sc.S + 1) * 4; }
};

// The outputs' places: the caller's own in device memory, else the workspace's.
int ol_place(wm_ctx *ctx, OutlierWs &w, OlCall &c) {
    const size_t n = c.n;
    WM_HIP(ctx, w.keep.reserve(n * 4));
    WM_HIP(ctx, w.pos.reserve((n + 1) * 4));
    WM_HIP(ctx, w.res.reserve(c.fetch_bytes()));
    WM_HIP(ctx, w.h_res.reserve(c.fetch_bytes()));
    if (c.labels_out) {
        if (c.host_out) WM_HIP(ctx, w.labels.reserve(n));
        c.d_labels = c.host_out ? w.labels.as<uint8_t>() : c.labels_out;
    }
    if (c.stat()) {
        if (c.host_out || !c.mean_dist_out) WM_HIP(ctx, w.dist.reserve(n * 4));
        c.d_dist = (c.host_out || !c.mean_dist_out) ? w.dist.as<float>() : c.mean_dist_out;
    } else {
        if (c.host_out || !c.counts_out) WM_HIP(ctx, w.counts.reserve(n * 4));
        c.d_counts = (c.host_out || !c.counts_out) ? w.counts.as<int>() : c.counts_out;
    }
    c.d_cap = std::min(c.cap, n);
    c.d_out = reinterpret_cast<int *>(c.indices_out);
    c.d_pout = static_cast<unsigned char *>(c.points_out);
    if (c.host_out) {
        WM_HIP(ctx, w.out.reserve(c.d_cap * 4));
        c.d_out = w.out.as<int>();
        if (c.points_out) {
            WM_HIP(ctx, w.pout.reserve(c.d_cap * c.out_stride));
            c.d_pout = w.pout.as<unsigned char>();
        }
    }
    return WM_OK;
}

// What a point without a search keeps: label NONE (k_outlier_label writes every label), distance 0, count -1.
int ol_defaults(wm_ctx *ctx, const OlCall &c) {
    if (c.stat() && c.mean_dist_out) WM_HIP(ctx, hipMemsetAsync(c.d_dist, 0, c.n * 4, ctx->stream));
    if (!c.stat() && c.counts_out) {
        hipLaunchKernelGGL(k_outlier_fill, dim3(c.blocks), dim3(kBlock), 0, ctx->stream, c.d_counts, (unsigned) c.n, -1);
        WM_HIP(ctx, hipGetLastError());
    }
    return WM_OK;
}

// Behind the stream's wait: the first m kept entries and the per-point arrays to a caller in host memory.
int ol_to_host(wm_ctx *ctx, const OlCall &c, size_t m) {
    if (!c.host_out) return WM_OK;
    if (m) WM_HIP(ctx, hipMemcpy(c.indices_out, c.d_out, m * 4, hipMemcpyDeviceToHost));
    if (m && c.points_out) WM_HIP(ctx, hipMemcpy(c.points_out, c.d_pout, m * c.out_stride, hipMemcpyDeviceToHost));
    if (c.labels_out) WM_HIP(ctx, hipMemcpy(c.labels_out, c.d_labels, c.n, hipMemcpyDeviceToHost));
    if (c.stat() && c.mean_dist_out) WM_HIP(ctx, hipMemcpy(c.mean_dist_out, c.d_dist, c.n * 4, hipMemcpyDeviceToHost));
    if (!c.stat() && c.counts_out) WM_HIP(ctx, hipMemcpy(c.counts_out, c.d_counts, c.n * 4, hipMemcpyDeviceToHost));
    return WM_OK;
}

// A call without a finite point: nothing to search, the outputs' defaults are the answer.
int ol_nothing_finite(wm_ctx *ctx, const OlCall &c) {
    WM_TRY(ol_defaults(ctx, c));
    if (c.labels_out) WM_HIP(ctx, hipMemsetAsync(c.d_labels, 0, c.n, ctx->stream));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ol_to_host(ctx, c, 0);
}

// Behind the grid: the searches, the thresholds, labels, the kept list, and the copies to the host.  The defaults, one
// memset of res, 5 launches of the statistical filter or 3 of the radius filter, one exclusive scan, ONE fetch (the
// statistics of all scans and the offsets behind them) and the wait at the end -- whatever the number of scans.
int ol_back(wm_ctx *ctx, OutlierWs &w, OlCall &c) {
    hipStream_t st = ctx->stream;
    const wm_outlier_params *p = c.p;
    const OlScans &sc = c.sc;
    const unsigned S = sc.S;
    const float4 *pts = w.sb.pts.as<float4>();
    double *res = w.res.as<double>();
    unsigned *offs = reinterpret_cast<unsigned *>(res + 4 * (size_t) S);

    WM_TRY(ol_defaults(ctx, c));
    WM_HIP(ctx, hipMemsetAsync(res, 0, c.res_bytes(), st));
    if (c.stat()) {
        const int k = p->mean_k + 1;
        const float r0 = ctx->tune_knn_r0 > 0 ? ctx->tune_knn_r0 : (k <= 12 ? 1.0f : 1.5f);
        if (c.search_blocks)
            knn_ladder(k, [&](auto K) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_mean_dist<decltype(K)::value>), dim3(c.search_blocks),
                                   dim3(kOutBlock), 0, st, sc, k, r0, c.d_dist);
            });
        if (c.rows) {
            WM_HIP(ctx, w.part.reserve((size_t) c.rows * 2 * sizeof(double)));
            hipLaunchKernelGGL(k_outlier_moments, dim3(c.rows), dim3(kBlock), 0, st, sc, pts, (const float *) c.d_dist,
                               w.part.as<double>());
            hipLaunchKernelGGL(k_outlier_threshold, dim3(S), dim3(64), 0, st, sc, (const double *) w.part.as<double>(),
                               p->stddev_mult, res);
        }
        WM_HIP(ctx, hipGetLastError());
    } else if (c.search_blocks) {
        const float r2 = (float) (p->radius * p->radius);
        const float rf = sqrtf(r2) * 1.0001f;  // (a point with float d2 < r2 lies within this of the query)
        const unsigned stop = (unsigned) p->min_neighbors + 1u;
        if (c.counts_out)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_radius<true>), dim3(c.search_blocks), dim3(kOutBlock), 0, st, sc, r2, rf,
                               stop, c.d_counts);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_radius<false>), dim3(c.search_blocks), dim3(kOutBlock), 0, st, sc, r2, rf,
                               stop, c.d_counts);
        WM_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_outlier_label, dim3(c.blocks), dim3(kBlock), 0, st, sc, pts, (const float *) c.d_dist,
                       c.stat() ? (const double *) res : (const double *) nullptr, (const int *) c.d_counts, p->min_neighbors,
                       p->negative, c.d_labels, w.keep.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, w.keep.as<unsigned>(), c.n, w.pos.as<unsigned>()));
    hipLaunchKernelGGL(k_outlier_emit, dim3(std::max(c.blocks, blocks_of((size_t) S + 1))), dim3(kBlock), 0, st, sc, c.blocks,
                       (unsigned) c.n, pts, (const unsigned *) w.keep.as<unsigned>(), (const unsigned *) w.pos.as<unsigned>(),
                       c.d_out, c.d_cap, c.d_pout, c.out_stride, offs);
    WM_HIP(ctx, hipGetLastError());
    if (c.timed) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipMemcpyAsync(w.h_res.p, res, c.fetch_bytes(), hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));

    if (c.timed) (void) hipEventElapsedTime(&c.ms, ctx->ev_a, ctx->ev_b);
    const double *h_res = w.h_res.as<double>();
    const unsigned *h_offs = reinterpret_cast<const unsigned *>(h_res + 4 * (size_t) S);
    for (unsigned k = 0; k <= S; ++k) c.offsets_out[k] = h_offs[k];
    const size_t kept = h_offs[S];
    if (c.stats)
        for (unsigned k = 0; k < S; ++k) {
            if (c.status && c.status[k] != WM_OK) continue;  // (zeroed apart from n_finite, as the single call leaves them)
            wm_outlier_stats &s = c.stats[k];
            const size_t kk = h_offs[k + 1] - h_offs[k], nf = c.h_tab ? c.h_tab[k].nf : sc.one.nf;
            s.n_inliers = p->negative ? nf - kk : kk;
            s.n_outliers = nf - s.n_inliers;
            s.mean = h_res[4 * (size_t) k];
            s.stddev = h_res[4 * (size_t) k + 1];
            s.threshold = h_res[4 * (size_t) k + 2];
            s.kernel_ms = c.ms;
        }
    WM_TRY(ol_to_host(ctx, c, std::min(kept, c.cap)));
    return kept > c.cap ? WM_ERR_ARG : WM_OK;
}

// One scan, handed to the kernels by value: no table, no staging.  This is wm_outlier_filter, and
// wm_outlier_filter_batch for a batch of one (arguments checked by the callers, the outputs zeroed, n > 0; `c` holds
// the parameters and the outputs).  WM_NOT_CONVERGED: fewer than mean_k + 1 finite points, nothing written.
int ol_one(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, OlCall &c) {
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->outlier) ctx->outlier = new OutlierWs();
    OutlierWs &w = *static_cast<OutlierWs *>(ctx->outlier);
    hipStream_t st = ctx->stream;
    c.n = n;
    c.blocks = blocks_of(n);
    WM_HIP(ctx, w.sb.pts.reserve(n * sizeof(float4)));
    WM_TRY(ol_place(ctx, w, c));

    if (c.timed) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, w.sb.pts.as<float4>()));
    Bbox bb;
    size_t n_finite = 0;
    WM_TRY(compute_bbox(ctx, w.sb.pts.as<float4>(), n, &bb, &n_finite));
    if (c.stats) c.stats->n_finite = n_finite;
    // PCL: "Number of points in cloud is less than mean_k": as the k-NN entry points
    if (c.stat() && n_finite > 0 && n_finite < (size_t) c.p->mean_k + 1) {
        WM_HIP(ctx, hipStreamSynchronize(st));
        return WM_NOT_CONVERGED;
    }
    if (n_finite == 0) return ol_nothing_finite(ctx, c);
    WM_TRY(build_call_grid(ctx, w.sb.pts.as<float4>(), n, n_finite, bb, ol_floor_h(ctx, c.p), &w.sb.grid));
    c.sc.one.n = (unsigned) n;
    c.sc.one.nf = c.sc.one.searched = (unsigned) n_finite;
    c.sc.one.g = w.sb.grid.d;
    c.search_blocks = (unsigned) ((n_finite + kOutBlock - 1) / kOutBlock);
    c.rows = c.stat() ? outlier_rows((unsigned) n, (unsigned) n_finite) : 0u;
    return ol_back(ctx, w, c);
}

// An output array of `bytes` bytes in `out_mem` set to zero (a batch's slices that carry no meaning).
int outlier_zero(wm_ctx *ctx, void *p, size_t bytes, bool host_out) {
    if (!p || !bytes) return WM_OK;
    if (host_out) memset(p, 0, bytes);
    else WM_HIP(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
    return WM_OK;
}

}  // namespace

}  // namespace wm

using namespace wm;

extern "C" {

void wm_outlier_default_params(wm_outlier_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->method = WM_OUTLIER_STATISTICAL;
    p->mean_k = 1;         // statistical_outlier_removal.h: mean_k_ (1), std_mul_ (0.0)
    p->stddev_mult = 0.0;
    p->radius = 0.0;       // radius_outlier_removal.h: search_radius_ (0.0), min_pts_radius_ (1)
    p->min_neighbors = 1;
    p->negative = 0;
}

int wm_outlier_filter(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_outlier_params *p,
                      int32_t *indices_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out,
                      float *mean_dist_out, int32_t *counts_out, wm_outlier_stats *stats) {
    if (!ctx || !p || !n_out || (n > 0 && !pts) || stride < 12 || (stride & 3) || n > 0x7FFFFFF0u ||
        (cap > 0 && !indices_out) || (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) ||
        (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE) || !outlier_params_ok(p))
        return WM_ERR_ARG;
    *n_out = 0;
    if (stats) *stats = wm_outlier_stats{};
    if (n == 0) return WM_OK;
    size_t offs[2] = {0, 0};
    OlCall c;
    c.p = p;
    c.host_out = out_mem == WM_MEM_HOST;
    c.timed = stats != nullptr;
    c.indices_out = indices_out;
    c.cap = cap;
    c.offsets_out = offs;
    c.labels_out = labels_out;
    c.mean_dist_out = mean_dist_out;
    c.counts_out = counts_out;
    c.stats = stats;
    const int rc = ol_one(ctx, pts, n, stride, mem, c);
    *n_out = offs[1];
    return rc;
}

int wm_outlier_filter_batch(wm_ctx *ctx, const wm_outlier_scan *scans, int n_scans, size_t stride, int mem,
                            const wm_outlier_params *p, int32_t *indices_out, size_t cap, void *points_out, size_t out_stride,
                            int out_mem, size_t *offsets_out, uint8_t *labels_out, float *mean_dist_out, int32_t *counts_out,
                            int *status, wm_outlier_stats *stats, float *kernel_ms) {
    if (!ctx || !p || n_scans < 0 || (n_scans > 0 && (!scans || !status)) || !offsets_out || stride < 12 || (stride & 3) ||
        (cap > 0 && !indices_out) || (points_out && (out_stride < 12 || (out_stride & 3))) ||
        (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) || (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE) ||
        !outlier_params_ok(p) || (unsigned long long) n_scans > WM_OUTLIER_BATCH_MAX_SCANS)
        return WM_ERR_ARG;
    const unsigned S = (unsigned) n_scans;
    size_t total = 0;
    for (unsigned k = 0; k < S; ++k) {
        if ((scans[k].n > 0 && !scans[k].pts) || scans[k].n > WM_OUTLIER_BATCH_MAX_POINTS) return WM_ERR_ARG;
        total += scans[k].n;
        if (total > WM_OUTLIER_BATCH_MAX_POINTS) return WM_ERR_ARG;
    }
    for (unsigned k = 0; k <= S; ++k) offsets_out[k] = 0;
    for (unsigned k = 0; k < S; ++k) status[k] = WM_OK;
    if (stats)
        for (unsigned k = 0; k < S; ++k) stats[k] = wm_outlier_stats{};
    if (kernel_ms) *kernel_ms = 0.f;
    if (S == 0 || total == 0) return WM_OK;  // (no device is touched)
    OlCall c;
    c.p = p;
    c.host_out = out_mem == WM_MEM_HOST;
    c.indices_out = indices_out;
    c.cap = cap;
    c.points_out = points_out;
    c.out_stride = points_out ? out_stride : 0;
    c.offsets_out = offsets_out;
    c.labels_out = labels_out;
    c.mean_dist_out = mean_dist_out;
    c.counts_out = counts_out;
    c.stats = stats;
    if (S == 1) {  // a batch of one is the single call: nothing to stage, nothing to amortise
        c.timed = stats || kernel_ms;
        const int rc = ol_one(ctx, scans[0].pts, total, stride, mem, c);
        if (kernel_ms) *kernel_ms = c.ms;
        if (rc != WM_NOT_CONVERGED) return rc;
        status[0] = rc;  // nothing was written: the slices hold 0 / NONE
        WM_TRY(outlier_zero(ctx, labels_out, total, c.host_out));
        WM_TRY(outlier_zero(ctx, mean_dist_out, total * 4, c.host_out));
        WM_TRY(outlier_zero(ctx, counts_out, total * 4, c.host_out));
        if (!c.host_out) WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WM_OK;
    }
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->outlier) ctx->outlier = new OutlierWs();
    OutlierWs &w = *static_cast<OutlierWs *>(ctx->outlier);

    // the front (wm_scan_batch.hpp).  A scan that is not converged is not searched; a searched scan of the statistical
    // filter gets its rows of the moment sums, first row in aux0
    const unsigned kmin = c.stat() ? (unsigned) p->mean_k + 1u : 0u;
    size_t rows = 0;
    ScanBatch b;
    WM_TRY(scan_batch_front(ctx, w.sb, scans, S, stride, mem, ol_floor_h(ctx, p), (unsigned) kOutBlock,
                            [&](unsigned k, ClScan &t) {
                                const bool searched = t.nf >= kmin;
                                if (!searched && t.nf) status[k] = WM_NOT_CONVERGED;
                                if (stats) stats[k].n_finite = t.nf;
                                t.aux0 = (unsigned) rows;
                                if (c.stat()) rows += outlier_rows(t.n, searched ? t.nf : 0u);
                                return searched;
                            },
                            &b));
    c.sc.tab = b.d_tab;
    c.sc.S = S;
    c.sc.one.g.pts = w.sb.grid.pts.as<float4>();
    c.sc.one.g.cell_start = w.sb.grid.cell_start.as<unsigned>();
    c.h_tab = b.tab;
    c.n = total;
    c.blocks = (unsigned) b.blocks;
    c.search_blocks = (unsigned) b.search_blocks;
    c.rows = (unsigned) rows;
    c.timed = true;  // (PairStage::submit records ev_a)
    c.status = status;
    WM_TRY(ol_place(ctx, w, c));
    if (b.nf_total == 0) return ol_nothing_finite(ctx, c);
    const int rc = ol_back(ctx, w, c);
    if (kernel_ms) *kernel_ms = c.ms;
    return rc;
}

}  // extern "C"
