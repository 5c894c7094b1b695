// wm_outlier.hip -- outlier removal on the device: pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval as one
// cloud-in / indices-out call (wm_outlier_filter), shaped like wm_ground_segment: the call packs the cloud, builds a
// cell-sorted grid over it for this call alone, and works in a workspace of its own on the context.
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
// Launches of a call: pack + bounding box, the grid (count, scan, scatter), then
//   statistical  k_outlier_mean_dist<K> (knn_search<K> straight into the mean distance: the lists never reach memory),
//                k_outlier_moments + k_outlier_threshold (the two sums in double, a fixed tree over the points in CALLER
//                order: the cell sort's order inside a cell is the atomics' arrival order and must not reach a sum)
//   radius       k_outlier_radius<EXACT> (one lane per query over the rows of the box [q - r, q + r])
//   both         k_outlier_label, exclusive_scan, k_outlier_compact (kept indices in ascending input order).
//
// A batch (wm_outlier_filter_batch; ClScan: a scan's row of the device table): every output of scan k EQUALS the
// single call's for that scan alone, bit for bit.  What that asks of the code:
//   front      wm_scan_batch.hpp's, shared with wm_cluster_extract_batch: batch positions (scan-major), a lattice per
//              scan under the shared 2^26-cell budget, ONE cell-sorted array.  Coarser cells change no output: the
//              searches below are exact whatever the lattice.
//   searches   a search workgroup is one wave of 64 queries of ONE scan, found from the table of first workgroups (as
//              k_cluster_link), and uses that scan's GridDev: a walk never meets a point of another scan.  knn_search<K>
//              and radius_walk are used as they are; .w is the batch position, monotonic in the caller index inside a
//              scan, so the (d2, index) tie order is the single call's.  The K ladder and its waves_per_eu attributes
//              are the single call's.  A scan that is not converged (0 < n_finite < mean_k + 1) gets no search
//              workgroup and no row of the moment sums; its labels are NONE and nothing of it is kept.
//   moments    the two sums are the single call's fixed tree over the scan's points in caller order, whose shape depends
//              on that scan's n alone: rows = min(blocks_of(n), 1024) workgroups of 256 threads, thread t takes points
//              t, t + rows * 256, ...; the wave's shuffle tree; thread 0 over the four waves; one wave over the rows.
//              Scan k gets exactly that: rows_k workgroups found through a table of first rows (ClScan::aux0), one
//              threshold wave per scan.  That makes mean, stddev and threshold bit-equal, and with them the labels.
//   atomics    no sum depends on the grid's arrival order; none runs through atomics over floats or doubles.
//   compaction k_outlier_label_batch over batch positions with the scan's own threshold, ONE exclusive scan over the
//              batch (a scan's offset is the scan's value at its first position), one k_outlier_emit writing indices
//              local to the scan and, if wanted, the points.
//   waits      the boxes' fetch, the occupancies' fetch and the final one; launches and waits do not depend on n_scans.
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

// ------------------------------------------------------------------ statistical: mean distance to the mean_k nearest
// Queries in the grid's own (cell-sorted) order -- a wave's 64 queries scan the same few rows of cells -- the result
// stored under the point's caller index (.w).  Only finite points are in the grid; k = mean_k + 1 <= their number.
template <int K>
__global__ void __launch_bounds__(kOutBlock) __attribute__((amdgpu_waves_per_eu(K <= 10 ? 6 : (K <= 12 ? 5 : 1))))
    k_outlier_mean_dist(GridDev g, unsigned n, int k, float r0_cells, float *__restrict__ dist_out) {
    __shared__ uint2 s_runs[kKnnRows * kOutBlock];
    const unsigned i = blockIdx.x * kOutBlock + threadIdx.x;
    if (i >= n) return;
    const float4 q = g.pts[i];
    unsigned long long best[K];
    knn_search<K>(g, q.x, q.y, q.z, k, r0_cells, best, s_runs, threadIdx.x, kOutBlock);
    double s = 0.0;
#pragma unroll
    for (int j = 1; j < K; ++j)
        if (j < k) s += sqrt((double) __uint_as_float((unsigned) (best[j] >> 32)));
    dist_out[__float_as_uint(q.w)] = (float) (s / (double) (k - 1));
}

// sum d and sum d^2 over the finite points, caller order: thread t of the launch takes points t, t + T, ...; a wave's
// 64 sums by a shuffle tree, a workgroup's four by thread 0 in wave order -> row blockIdx.x of `part`
__global__ void __launch_bounds__(kBlock)
    k_outlier_moments(const float4 *__restrict__ pts, const float *__restrict__ dist, unsigned n, double *__restrict__ part) {
    double s1 = 0.0, s2 = 0.0;
    const unsigned stride = gridDim.x * kBlock;
    for (unsigned i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float x = pts[i].x;
        if (x == x) {
            const double d = (double) dist[i];
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
        part[2 * blockIdx.x] = s1;
        part[2 * blockIdx.x + 1] = s2;
    }
}

// the rows added in one fixed order (one wave: lane l takes rows l, l + 64, ..., then the shuffle tree) ->
// res[0] mean, [1] stddev, [2] threshold
__global__ void __launch_bounds__(64)
    k_outlier_threshold(const double *__restrict__ part, unsigned rows, double n_finite, double stddev_mult,
                        double *__restrict__ res) {
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
        const double mean = s1 / n_finite;
        const double var = (s2 - s1 * s1 / n_finite) / (n_finite - 1.0);
        const double sd = sqrt(var);
        res[0] = mean;
        res[1] = sd;
        res[2] = mean + stddev_mult * sd;
    }
}

// ------------------------------------------------------------------ radius: neighbours within r
// One lane per query (grid order, result under .w) over the rows of the box of cells covering [q - r, q + r]:
// radius_walk (wm_radius_walk.hpp, shared with k_cluster_link).  hits counts d2 < r2, the query itself among them
// (d2 = 0) whenever r2 > 0; the count written is the OTHER points'.
// EXACT: the count is exact.  Otherwise a lane stops once it has seen `stop` hits (min_neighbors + 1, itself
// included): what it writes then is >= min_neighbors, which is all the labelling asks.
template <bool EXACT>
__global__ void __launch_bounds__(kOutBlock)
    k_outlier_radius(GridDev g, unsigned n, float r2, float r_cells, unsigned stop, int *__restrict__ count_out) {
    __shared__ uint2 s_runs[kKnnRows * kOutBlock];
    const unsigned i = blockIdx.x * kOutBlock + threadIdx.x;
    if (i >= n) return;
    const float4 q = g.pts[i];
    unsigned hits = 0;
    radius_walk<!EXACT>(g, q, r_cells, s_runs, threadIdx.x, kOutBlock, [&](unsigned, const float4 &t) {
        hits += g_d2(q.x, q.y, q.z, t) < r2 ? 1u : 0u;
        return !EXACT && hits >= stop;
    });
    const unsigned self = r2 > 0.f ? 1u : 0u;
    count_out[__float_as_uint(q.w)] = (int) (hits - (hits >= self ? self : 0u));
}

// ------------------------------------------------------------------ labels and the kept list (caller order)
// `thr`: the statistical filter's threshold in device memory (res[2]), nullptr for the radius filter
__global__ void __launch_bounds__(kBlock)
    k_outlier_label(const float4 *__restrict__ pts, unsigned n, const float *__restrict__ dist, const double *__restrict__ thr,
                    const int *__restrict__ counts, int min_neighbors, int negative, uint8_t *__restrict__ labels,
                    unsigned *__restrict__ keep) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float x = pts[i].x;
    const bool finite = x == x;
    bool outlier = false;
    if (finite) outlier = thr ? (double) dist[i] > *thr : counts[i] < min_neighbors;
    if (labels) labels[i] = finite ? (outlier ? WM_OUTLIER_OUTLIER : WM_OUTLIER_INLIER) : WM_OUTLIER_NONE;
    keep[i] = finite && outlier == (negative != 0) ? 1u : 0u;
}

// pos = the exclusive scan of keep (n + 1 entries); res[3] = the number kept
__global__ void __launch_bounds__(kBlock)
    k_outlier_compact(const unsigned *__restrict__ keep, const unsigned *__restrict__ pos, unsigned n, int *__restrict__ out,
                      size_t cap, double *__restrict__ res) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) res[3] = (double) pos[n];
    if (i >= n) return;
    if (keep[i] && pos[i] < cap) out[pos[i]] = (int) i;
}

__global__ void __launch_bounds__(kBlock) k_outlier_fill(int *__restrict__ p, unsigned n, int v) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ a batch: the same steps with a scan dimension
// k_outlier_mean_dist for the wave's scan: its lattice, its grid positions, its k <= its finite points
template <int K>
__global__ void __launch_bounds__(kOutBlock) __attribute__((amdgpu_waves_per_eu(K <= 10 ? 6 : (K <= 12 ? 5 : 1))))
    k_outlier_mean_dist_batch(const ClScan *__restrict__ tab, unsigned S, int k, float r0_cells, float *__restrict__ dist_out) {
    __shared__ uint2 s_runs[kKnnRows * kOutBlock];
    const unsigned s = cl_by_search(tab, S, blockIdx.x);
    const GridDev g = tab[s].g;
    const unsigned i = tab[s].g0 + (blockIdx.x - tab[s].lblk0) * kOutBlock + threadIdx.x;
    if (i >= tab[s].g0 + tab[s].searched) return;
    const float4 q = g.pts[i];
    unsigned long long best[K];
    knn_search<K>(g, q.x, q.y, q.z, k, r0_cells, best, s_runs, threadIdx.x, kOutBlock);
    double sum = 0.0;
#pragma unroll
    for (int j = 1; j < K; ++j)
        if (j < k) sum += sqrt((double) __uint_as_float((unsigned) (best[j] >> 32)));
    dist_out[__float_as_uint(q.w)] = (float) (sum / (double) (k - 1));
}

// the scan's rows of the moment sums: min(blocks_of(n), kMomBlocksMax) for a searched scan, else none
__host__ __device__ __forceinline__ unsigned outlier_rows(unsigned n, unsigned searched) {
    const unsigned b = (n + kBlock - 1) / kBlock;
    return searched ? (b < (unsigned) kMomBlocksMax ? b : (unsigned) kMomBlocksMax) : 0u;
}

// k_outlier_moments, row (blockIdx.x - aux0) of the scan's own tree -> row blockIdx.x of `part`
__global__ void __launch_bounds__(kBlock)
    k_outlier_moments_batch(const ClScan *__restrict__ tab, unsigned S, const float4 *__restrict__ pts,
                            const float *__restrict__ dist, double *__restrict__ part) {
    const unsigned k = cl_find(tab, S, blockIdx.x, [](const ClScan &s) { return s.aux0; });
    const ClScan me = tab[k];
    const unsigned rows = outlier_rows(me.n, me.searched);
    const unsigned row = blockIdx.x - me.aux0;
    double s1 = 0.0, s2 = 0.0;
    const unsigned stride = rows * kBlock;
    for (unsigned i = row * kBlock + threadIdx.x; i < me.n; i += stride) {
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

// k_outlier_threshold, one wave per scan (blockIdx.x) over the scan's rows -> res[4 k]: mean, stddev, threshold; a
// scan without rows (empty, nothing finite, not converged) keeps the zeros res was cleared to
__global__ void __launch_bounds__(64)
    k_outlier_threshold_batch(const ClScan *__restrict__ tab, const double *__restrict__ part, double stddev_mult,
                              double *__restrict__ res) {
    const ClScan me = tab[blockIdx.x];
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

// k_outlier_radius for the wave's scan
template <bool EXACT>
__global__ void __launch_bounds__(kOutBlock)
    k_outlier_radius_batch(const ClScan *__restrict__ tab, unsigned S, float r2, float rf, unsigned stop, int *__restrict__ count_out) {
    __shared__ uint2 s_runs[kKnnRows * kOutBlock];
    const unsigned s = cl_by_search(tab, S, blockIdx.x);
    const GridDev g = tab[s].g;
    const unsigned i = tab[s].g0 + (blockIdx.x - tab[s].lblk0) * kOutBlock + threadIdx.x;
    if (i >= tab[s].g0 + tab[s].searched) return;
    const float4 q = g.pts[i];
    unsigned hits = 0;
    radius_walk<!EXACT>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kOutBlock, [&](unsigned, const float4 &t) {
        hits += g_d2(q.x, q.y, q.z, t) < r2 ? 1u : 0u;
        return !EXACT && hits >= stop;
    });
    const unsigned self = r2 > 0.f ? 1u : 0u;
    count_out[__float_as_uint(q.w)] = (int) (hits - (hits >= self ? self : 0u));
}

// k_outlier_label over batch positions: a workgroup belongs to one scan and reads that scan's threshold (res[4 k + 2];
// res == nullptr: the radius filter).  A scan with finite points that is not searched is not converged: NONE, not kept.
__global__ void __launch_bounds__(kBlock)
    k_outlier_label_batch(const ClScan *__restrict__ tab, unsigned S, const float4 *__restrict__ pts,
                          const float *__restrict__ dist, const double *__restrict__ res, const int *__restrict__ counts,
                          int min_neighbors, int negative, uint8_t *__restrict__ labels, unsigned *__restrict__ keep) {
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
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

// pos = the exclusive scan of keep over the batch (total + 1 entries).  offs[k] = pos at scan k's first position,
// offs[S] = the number kept; a kept point: its index inside its scan and, for points_out, its x y z as the packed
// cloud holds them (a kept point is finite, and a finite point is packed bit for bit) in records of out_stride bytes,
// the bytes behind z zero (k_cluster_emit's rules).
__global__ void __launch_bounds__(kBlock)
    k_outlier_emit(const ClScan *__restrict__ tab, unsigned S, unsigned blocks, unsigned total, const float4 *__restrict__ pts,
                   const unsigned *__restrict__ keep, const unsigned *__restrict__ pos, int *__restrict__ out, size_t cap,
                   unsigned char *__restrict__ pout, size_t out_stride, unsigned *__restrict__ offs) {
    const size_t t = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (t <= S) offs[t] = pos[t < S ? tab[t].off : total];
    if (blockIdx.x >= blocks) return;
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
    const unsigned li = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    if (li >= me.n) return;
    const unsigned i = me.off + li;
    if (!keep[i]) return;
    const unsigned j = pos[i];
    if (j >= cap) return;
    out[j] = (int) li;
    if (pout) {
        const float4 v = pts[i];
        unsigned *o = reinterpret_cast<unsigned *>(pout + (size_t) j * out_stride);
        o[0] = __float_as_uint(v.x);
        o[1] = __float_as_uint(v.y);
        o[2] = __float_as_uint(v.z);
        for (size_t w = 3; w < out_stride / 4; ++w) o[w] = 0u;
    }
}

// a batch of one with points_out: the single call's kept list (caller indices) -> the points, k_outlier_emit's records
__global__ void __launch_bounds__(kBlock)
    k_outlier_gather(const float4 *__restrict__ pts, const int *__restrict__ idx, unsigned m, unsigned char *__restrict__ pout,
                     size_t out_stride) {
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const float4 v = pts[idx[j]];
    unsigned *o = reinterpret_cast<unsigned *>(pout + (size_t) j * out_stride);
    o[0] = __float_as_uint(v.x);
    o[1] = __float_as_uint(v.y);
    o[2] = __float_as_uint(v.z);
    for (size_t w = 3; w < out_stride / 4; ++w) o[w] = 0u;
}

}  // namespace

// The context's workspace of this filter: its own buffers, shared with nothing else on the context.
struct OutlierWs {
    DevBuf dist, counts, labels, keep, pos, out, part, res;
    DevBuf pout, offs;  // a batch: host points on their way; the scans' offsets
    ScanBatchBufs sb;   // the packed cloud and its grid; a batch's front (wm_scan_batch.hpp)
    PinnedBuf h_batch;  // a batch: mean, stddev, threshold per scan, then the offsets
    double *h_res = nullptr;  // pinned: mean, stddev, threshold, kept
};

void outlier_release(wm_ctx *ctx) {
    OutlierWs *w = static_cast<OutlierWs *>(ctx->outlier);
    if (!w) return;
    DevBuf *bufs[] = {&w->dist, &w->counts, &w->labels, &w->keep, &w->pos, &w->out, &w->part, &w->res, &w->pout, &w->offs};
    for (DevBuf *b : bufs) b->release();
    w->sb.release();
    w->h_batch.release();
    if (w->h_res) (void) hipHostFree(w->h_res);
    delete w;
    ctx->outlier = nullptr;
}

namespace {

template <int K>
int launch_mean_dist(wm_ctx *ctx, const GridDev &g, size_t n, int k, float *dist) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_mean_dist<K>), dim3((unsigned) ((n + kOutBlock - 1) / kOutBlock)),
                       dim3(kOutBlock), 0, ctx->stream, g, (unsigned) n, k,
                       ctx->tune_knn_r0 > 0 ? ctx->tune_knn_r0 : (k <= 12 ? 1.0f : 1.5f), dist);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// the K ladder of launch_cov_k / launch_debug_knn_k (wm_gicp.hip)
int launch_mean_dist_k(wm_ctx *ctx, const GridDev &g, size_t n, int k, float *dist) {
    if (k <= 8) return launch_mean_dist<8>(ctx, g, n, k, dist);
    if (k <= 10) return launch_mean_dist<10>(ctx, g, n, k, dist);
    if (k <= 12) return launch_mean_dist<12>(ctx, g, n, k, dist);
    if (k <= 16) return launch_mean_dist<16>(ctx, g, n, k, dist);
    if (k <= 20) return launch_mean_dist<20>(ctx, g, n, k, dist);
    if (k <= 24) return launch_mean_dist<24>(ctx, g, n, k, dist);
    return launch_mean_dist<32>(ctx, g, n, k, dist);
}

template <int K>
int launch_mean_dist_batch(wm_ctx *ctx, const ScanBatch &b, int k, float *dist) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_mean_dist_batch<K>), dim3((unsigned) b.search_blocks), dim3(kOutBlock), 0,
                       ctx->stream, b.d_tab, b.S, k, ctx->tune_knn_r0 > 0 ? ctx->tune_knn_r0 : (k <= 12 ? 1.0f : 1.5f), dist);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

int launch_mean_dist_batch_k(wm_ctx *ctx, const ScanBatch &b, int k, float *dist) {  // (launch_mean_dist_k's ladder)
    if (k <= 8) return launch_mean_dist_batch<8>(ctx, b, k, dist);
    if (k <= 10) return launch_mean_dist_batch<10>(ctx, b, k, dist);
    if (k <= 12) return launch_mean_dist_batch<12>(ctx, b, k, dist);
    if (k <= 16) return launch_mean_dist_batch<16>(ctx, b, k, dist);
    if (k <= 20) return launch_mean_dist_batch<20>(ctx, b, k, dist);
    if (k <= 24) return launch_mean_dist_batch<24>(ctx, b, k, dist);
    return launch_mean_dist_batch<32>(ctx, b, k, dist);
}

bool outlier_params_ok(const wm_outlier_params *p) {
    if (p->method == WM_OUTLIER_STATISTICAL) return p->mean_k >= 1 && p->mean_k <= 31;
    if (p->method == WM_OUTLIER_RADIUS) return std::isfinite(p->radius) && p->radius > 0 && p->min_neighbors >= 0;
    return false;
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

// An output array of `bytes` bytes in `out_mem` set to zero (a batch's slices that carry no meaning).
int outlier_zero(wm_ctx *ctx, void *p, size_t bytes, bool host_out) {
    if (!p || !bytes) return WM_OK;
    if (host_out) memset(p, 0, bytes);
    else WM_HIP(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
    return WM_OK;
}

// A batch of one scan is the single call; its points, if wanted, are gathered from the call's packed cloud.
int outlier_batch_of_one(wm_ctx *ctx, const wm_outlier_scan &scan, size_t stride, int mem, const wm_outlier_params *p,
                         int32_t *indices_out, size_t cap, void *points_out, size_t out_stride, int out_mem,
                         size_t *offsets_out, uint8_t *labels_out, float *mean_dist_out, int32_t *counts_out, int *status,
                         wm_outlier_stats *stats, float *kernel_ms) {
    const bool host_out = out_mem == WM_MEM_HOST;
    const size_t n = scan.n;
    wm_outlier_stats own{};
    wm_outlier_stats *s = stats ? stats : (kernel_ms ? &own : nullptr);
    size_t m = 0;
    const int rc = wm_outlier_filter(ctx, scan.pts, n, stride, mem, p, indices_out, cap, out_mem, &m, labels_out,
                                     mean_dist_out, counts_out, s);
    if (rc == WM_NOT_CONVERGED) {  // nothing was written: the slices hold 0 / NONE
        status[0] = rc;
        WM_TRY(outlier_zero(ctx, labels_out, n, host_out));
        WM_TRY(outlier_zero(ctx, mean_dist_out, n * 4, host_out));
        WM_TRY(outlier_zero(ctx, counts_out, n * 4, host_out));
        if (!host_out) WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WM_OK;
    }
    if (rc != WM_OK && rc != WM_ERR_ARG) return rc;
    offsets_out[1] = m;
    if (kernel_ms && s) *kernel_ms = s->kernel_ms;
    const size_t mw = std::min(m, cap);
    if (points_out && mw) {
        OutlierWs &w = *static_cast<OutlierWs *>(ctx->outlier);
        unsigned char *d_pout = static_cast<unsigned char *>(points_out);
        if (host_out) {
            WM_HIP(ctx, w.pout.reserve(mw * out_stride));
            d_pout = w.pout.as<unsigned char>();
        }
        hipLaunchKernelGGL(k_outlier_gather, dim3(blocks_of(mw)), dim3(kBlock), 0, ctx->stream,
                           (const float4 *) w.sb.pts.as<float4>(), host_out ? (const int *) w.out.as<int>() : (const int *) indices_out,
                           (unsigned) mw, d_pout, out_stride);
        WM_HIP(ctx, hipGetLastError());
        WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (host_out) WM_HIP(ctx, hipMemcpy(points_out, d_pout, mw * out_stride, hipMemcpyDeviceToHost));
    }
    return rc;
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
    const bool stat = p->method == WM_OUTLIER_STATISTICAL;
    const bool host_out = out_mem == WM_MEM_HOST;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->outlier) ctx->outlier = new OutlierWs();
    OutlierWs &w = *static_cast<OutlierWs *>(ctx->outlier);
    if (!w.h_res) WM_HIP(ctx, hipHostMalloc((void **) &w.h_res, 4 * sizeof(double), hipHostMallocDefault));
    hipStream_t st = ctx->stream;
    const unsigned nblocks = (unsigned) ((n + kBlock - 1) / kBlock);

    // the outputs' places: the caller's own in device memory, else the workspace's
    WM_HIP(ctx, w.sb.pts.reserve(n * sizeof(float4)));
    WM_HIP(ctx, w.keep.reserve(n * 4));
    WM_HIP(ctx, w.pos.reserve((n + 1) * 4));
    WM_HIP(ctx, w.res.reserve(4 * sizeof(double)));
    uint8_t *d_labels = nullptr;
    if (labels_out) {
        if (host_out) WM_HIP(ctx, w.labels.reserve(n));
        d_labels = host_out ? w.labels.as<uint8_t>() : labels_out;
    }
    float *d_dist = nullptr;
    int *d_counts = nullptr;
    if (stat) {
        if (host_out || !mean_dist_out) WM_HIP(ctx, w.dist.reserve(n * 4));
        d_dist = (host_out || !mean_dist_out) ? w.dist.as<float>() : mean_dist_out;
    } else {
        if (host_out || !counts_out) WM_HIP(ctx, w.counts.reserve(n * 4));
        d_counts = (host_out || !counts_out) ? w.counts.as<int>() : counts_out;
    }
    int *d_out = reinterpret_cast<int *>(indices_out);
    size_t d_cap = cap;
    if (host_out) {
        WM_HIP(ctx, w.out.reserve(n * 4));
        d_out = w.out.as<int>();
        d_cap = n;
    }

    if (stats) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, w.sb.pts.as<float4>()));
    Bbox bb;
    size_t n_finite = 0;
    WM_TRY(compute_bbox(ctx, w.sb.pts.as<float4>(), n, &bb, &n_finite));
    if (stats) stats->n_finite = n_finite;
    // PCL: "Number of points in cloud is less than mean_k": as the k-NN entry points, nothing written
    if (stat && n_finite > 0 && n_finite < (size_t) p->mean_k + 1) {
        WM_HIP(ctx, hipStreamSynchronize(st));
        return WM_NOT_CONVERGED;
    }
    // what a non-finite point keeps: label NONE (k_outlier_label writes every label), distance 0, count -1
    if (stat && mean_dist_out) WM_HIP(ctx, hipMemsetAsync(d_dist, 0, n * 4, st));
    if (!stat && counts_out) {
        hipLaunchKernelGGL(k_outlier_fill, dim3(nblocks), dim3(kBlock), 0, st, d_counts, (unsigned) n, -1);
        WM_HIP(ctx, hipGetLastError());
    }
    if (n_finite == 0) {  // nothing to search: the outputs' defaults are the answer
        if (labels_out) WM_HIP(ctx, hipMemsetAsync(d_labels, 0, n, st));
        WM_HIP(ctx, hipStreamSynchronize(st));
        if (host_out) {
            if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, n, hipMemcpyDeviceToHost));
            if (stat && mean_dist_out) WM_HIP(ctx, hipMemcpy(mean_dist_out, d_dist, n * 4, hipMemcpyDeviceToHost));
            if (!stat && counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, n * 4, hipMemcpyDeviceToHost));
        }
        return WM_OK;
    }

    float r2 = 0.f, rf = 0.f;
    if (!stat) {
        r2 = (float) (p->radius * p->radius);
        rf = sqrtf(r2) * 1.0001f;  // (a point with float d2 < r2 lies within this of the query)
    }
    const float div = ctx->tune_outlier_cell_div;
    // (the radius filter's box [q - r, q + r] must span a bounded number of rows: DESIGN.md 4.8 has the measurements)
    WM_TRY(build_call_grid(ctx, w.sb.pts.as<float4>(), n, n_finite, bb, stat ? 0.f : fminf((float) p->radius, 1.0e30f) / div,
                           &w.sb.grid));
    const GridDev &g = w.sb.grid.d;

    WM_HIP(ctx, hipMemsetAsync(w.res.p, 0, 4 * sizeof(double), st));
    if (stat) {
        WM_TRY(launch_mean_dist_k(ctx, g, n_finite, p->mean_k + 1, d_dist));
        const unsigned rows = std::min<unsigned>(nblocks, (unsigned) kMomBlocksMax);
        WM_HIP(ctx, w.part.reserve((size_t) rows * 2 * sizeof(double)));
        hipLaunchKernelGGL(k_outlier_moments, dim3(rows), dim3(kBlock), 0, st, w.sb.pts.as<float4>(), (const float *) d_dist,
                           (unsigned) n, w.part.as<double>());
        hipLaunchKernelGGL(k_outlier_threshold, dim3(1), dim3(64), 0, st, w.part.as<double>(), rows, (double) n_finite,
                           p->stddev_mult, w.res.as<double>());
        WM_HIP(ctx, hipGetLastError());
    } else {
        const unsigned sblocks = (unsigned) ((n_finite + kOutBlock - 1) / kOutBlock);
        const float r_cells = rf * g.inv_h;
        const unsigned stop = (unsigned) p->min_neighbors + 1u;
        if (counts_out)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_radius<true>), dim3(sblocks), dim3(kOutBlock), 0, st, g,
                               (unsigned) n_finite, r2, r_cells, stop, d_counts);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_radius<false>), dim3(sblocks), dim3(kOutBlock), 0, st, g,
                               (unsigned) n_finite, r2, r_cells, stop, d_counts);
        WM_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_outlier_label, dim3(nblocks), dim3(kBlock), 0, st, w.sb.pts.as<float4>(), (unsigned) n,
                       (const float *) d_dist, stat ? w.res.as<double>() + 2 : (const double *) nullptr,
                       (const int *) d_counts, p->min_neighbors, p->negative, d_labels, w.keep.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, w.keep.as<unsigned>(), n, w.pos.as<unsigned>()));
    hipLaunchKernelGGL(k_outlier_compact, dim3(nblocks), dim3(kBlock), 0, st, w.keep.as<unsigned>(), w.pos.as<unsigned>(),
                       (unsigned) n, d_out, d_cap, w.res.as<double>());
    WM_HIP(ctx, hipGetLastError());
    if (stats) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipMemcpyAsync(w.h_res, w.res.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));

    const size_t kept = (size_t) w.h_res[3];
    *n_out = kept;
    if (stats) {
        stats->n_inliers = p->negative ? n_finite - kept : kept;
        stats->n_outliers = n_finite - stats->n_inliers;
        stats->mean = w.h_res[0];
        stats->stddev = w.h_res[1];
        stats->threshold = w.h_res[2];
        (void) hipEventElapsedTime(&stats->kernel_ms, ctx->ev_a, ctx->ev_b);
    }
    if (host_out) {
        const size_t m = std::min(kept, cap);
        if (m) WM_HIP(ctx, hipMemcpy(indices_out, d_out, m * 4, hipMemcpyDeviceToHost));
        if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, n, hipMemcpyDeviceToHost));
        if (stat && mean_dist_out) WM_HIP(ctx, hipMemcpy(mean_dist_out, d_dist, n * 4, hipMemcpyDeviceToHost));
        if (!stat && counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, n * 4, hipMemcpyDeviceToHost));
    }
    return kept > cap ? WM_ERR_ARG : WM_OK;
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
    if (S == 1)
        return outlier_batch_of_one(ctx, scans[0], stride, mem, p, indices_out, cap, points_out, out_stride, out_mem,
                                    offsets_out, labels_out, mean_dist_out, counts_out, status, stats, kernel_ms);
    const bool stat = p->method == WM_OUTLIER_STATISTICAL;
    const bool host_out = out_mem == WM_MEM_HOST;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->outlier) ctx->outlier = new OutlierWs();
    OutlierWs &w = *static_cast<OutlierWs *>(ctx->outlier);
    hipStream_t st = ctx->stream;

    // the front (wm_scan_batch.hpp).  A scan that is not converged is not searched; a searched scan of the statistical
    // filter gets its rows of the moment sums, first row in aux0
    const unsigned kmin = stat ? (unsigned) p->mean_k + 1u : 0u;
    size_t rows = 0;
    float r2 = 0.f, rf = 0.f;
    if (!stat) {
        r2 = (float) (p->radius * p->radius);
        rf = sqrtf(r2) * 1.0001f;  // (a point with float d2 < r2 lies within this of the query)
    }
    ScanBatch b;
    WM_TRY(scan_batch_front(ctx, w.sb, scans, S, stride, mem,
                            stat ? 0.f : fminf((float) p->radius, 1.0e30f) / ctx->tune_outlier_cell_div, (unsigned) kOutBlock,
                            [&](unsigned k, ClScan &t) {
                                const bool searched = t.nf >= kmin;
                                if (!searched && t.nf) status[k] = WM_NOT_CONVERGED;
                                if (stats) stats[k].n_finite = t.nf;
                                t.aux0 = (unsigned) rows;
                                if (stat) rows += outlier_rows(t.n, searched ? t.nf : 0u);
                                return searched;
                            },
                            &b));
    const ClScan *tab = b.tab;
    const unsigned blocks = (unsigned) b.blocks;

    // the outputs' places: the caller's own in device memory, else the workspace's
    WM_HIP(ctx, w.keep.reserve(total * 4));
    WM_HIP(ctx, w.pos.reserve((total + 1) * 4));
    WM_HIP(ctx, w.res.reserve((size_t) S * 4 * sizeof(double)));
    WM_HIP(ctx, w.offs.reserve(((size_t) S + 1) * 4));
    const size_t res_bytes = (size_t) S * 4 * sizeof(double), offs_bytes = ((size_t) S + 1) * 4;
    WM_HIP(ctx, w.h_batch.reserve(res_bytes + offs_bytes));
    uint8_t *d_labels = nullptr;
    if (labels_out) {
        if (host_out) WM_HIP(ctx, w.labels.reserve(total));
        d_labels = host_out ? w.labels.as<uint8_t>() : labels_out;
    }
    float *d_dist = nullptr;
    int *d_counts = nullptr;
    if (stat) {
        if (host_out || !mean_dist_out) WM_HIP(ctx, w.dist.reserve(total * 4));
        d_dist = (host_out || !mean_dist_out) ? w.dist.as<float>() : mean_dist_out;
    } else {
        if (host_out || !counts_out) WM_HIP(ctx, w.counts.reserve(total * 4));
        d_counts = (host_out || !counts_out) ? w.counts.as<int>() : counts_out;
    }
    const size_t d_cap = std::min(cap, total);
    int *d_out = reinterpret_cast<int *>(indices_out);
    unsigned char *d_pout = static_cast<unsigned char *>(points_out);
    if (host_out) {
        WM_HIP(ctx, w.out.reserve(d_cap * 4));
        d_out = w.out.as<int>();
        if (points_out) {
            WM_HIP(ctx, w.pout.reserve(d_cap * out_stride));
            d_pout = w.pout.as<unsigned char>();
        }
    }

    // what a point without a search keeps: label NONE (k_outlier_label_batch writes every label), distance 0, count -1
    if (stat && mean_dist_out) WM_HIP(ctx, hipMemsetAsync(d_dist, 0, total * 4, st));
    if (!stat && counts_out) {
        hipLaunchKernelGGL(k_outlier_fill, dim3(blocks), dim3(kBlock), 0, st, d_counts, (unsigned) total, -1);
        WM_HIP(ctx, hipGetLastError());
    }
    if (b.nf_total == 0) {  // nothing to search: the outputs' defaults are the answer
        if (labels_out) WM_HIP(ctx, hipMemsetAsync(d_labels, 0, total, st));
        WM_HIP(ctx, hipStreamSynchronize(st));
        if (host_out) {
            if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, total, hipMemcpyDeviceToHost));
            if (stat && mean_dist_out) WM_HIP(ctx, hipMemcpy(mean_dist_out, d_dist, total * 4, hipMemcpyDeviceToHost));
            if (!stat && counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, total * 4, hipMemcpyDeviceToHost));
        }
        return WM_OK;
    }

    WM_HIP(ctx, hipMemsetAsync(w.res.p, 0, res_bytes, st));
    if (stat) {
        if (b.search_blocks) WM_TRY(launch_mean_dist_batch_k(ctx, b, p->mean_k + 1, d_dist));
        if (rows) {
            WM_HIP(ctx, w.part.reserve(rows * 2 * sizeof(double)));
            hipLaunchKernelGGL(k_outlier_moments_batch, dim3((unsigned) rows), dim3(kBlock), 0, st, b.d_tab, S,
                               (const float4 *) w.sb.pts.as<float4>(), (const float *) d_dist, w.part.as<double>());
            hipLaunchKernelGGL(k_outlier_threshold_batch, dim3(S), dim3(64), 0, st, b.d_tab, (const double *) w.part.as<double>(),
                               p->stddev_mult, w.res.as<double>());
            WM_HIP(ctx, hipGetLastError());
        }
    } else if (b.search_blocks) {
        const unsigned stop = (unsigned) p->min_neighbors + 1u;
        if (counts_out)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_radius_batch<true>), dim3((unsigned) b.search_blocks), dim3(kOutBlock), 0,
                               st, b.d_tab, S, r2, rf, stop, d_counts);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_outlier_radius_batch<false>), dim3((unsigned) b.search_blocks), dim3(kOutBlock), 0,
                               st, b.d_tab, S, r2, rf, stop, d_counts);
        WM_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_outlier_label_batch, dim3(blocks), dim3(kBlock), 0, st, b.d_tab, S, (const float4 *) w.sb.pts.as<float4>(),
                       (const float *) d_dist, stat ? (const double *) w.res.as<double>() : (const double *) nullptr,
                       (const int *) d_counts, p->min_neighbors, p->negative, d_labels, w.keep.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, w.keep.as<unsigned>(), total, w.pos.as<unsigned>()));
    hipLaunchKernelGGL(k_outlier_emit, dim3(std::max(blocks, blocks_of((size_t) S + 1))), dim3(kBlock), 0, st, b.d_tab, S, blocks,
                       (unsigned) total, (const float4 *) w.sb.pts.as<float4>(), (const unsigned *) w.keep.as<unsigned>(),
                       (const unsigned *) w.pos.as<unsigned>(), d_out, d_cap, d_pout, points_out ? out_stride : (size_t) 0,
                       w.offs.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    unsigned char *h = w.h_batch.as<unsigned char>();
    WM_HIP(ctx, hipMemcpyAsync(h, w.res.p, res_bytes, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipMemcpyAsync(h + res_bytes, w.offs.p, offs_bytes, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));

    float ms = 0.f;
    (void) hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b);
    if (kernel_ms) *kernel_ms = ms;
    const double *h_res = reinterpret_cast<const double *>(h);
    const unsigned *h_offs = reinterpret_cast<const unsigned *>(h + res_bytes);
    for (unsigned k = 0; k <= S; ++k) offsets_out[k] = h_offs[k];
    const size_t kept = h_offs[S];
    if (stats)
        for (unsigned k = 0; k < S; ++k) {
            if (status[k] != WM_OK) continue;  // (zeroed apart from n_finite, as the single call leaves them)
            const size_t kk = h_offs[k + 1] - h_offs[k], nf = tab[k].nf;
            stats[k].n_inliers = p->negative ? nf - kk : kk;
            stats[k].n_outliers = nf - stats[k].n_inliers;
            stats[k].mean = h_res[4 * (size_t) k];
            stats[k].stddev = h_res[4 * (size_t) k + 1];
            stats[k].threshold = h_res[4 * (size_t) k + 2];
            stats[k].kernel_ms = ms;
        }
    if (host_out) {
        const size_t m = std::min(kept, cap);
        if (m) WM_HIP(ctx, hipMemcpy(indices_out, d_out, m * 4, hipMemcpyDeviceToHost));
        if (m && points_out) WM_HIP(ctx, hipMemcpy(points_out, d_pout, m * out_stride, hipMemcpyDeviceToHost));
        if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, total, hipMemcpyDeviceToHost));
        if (stat && mean_dist_out) WM_HIP(ctx, hipMemcpy(mean_dist_out, d_dist, total * 4, hipMemcpyDeviceToHost));
        if (!stat && counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, total * 4, hipMemcpyDeviceToHost));
    }
    return kept > cap ? WM_ERR_ARG : WM_OK;
}

}  // extern "C"
