// wm_cluster.hip -- Euclidean cluster extraction on the device: pcl::EuclideanClusterExtraction as one cloud-in /
// clusters-out call (wm_cluster_extract), shaped like wm_outlier_filter: the call packs the cloud, builds a cell-sorted
// grid over it for this call alone, and works in a workspace of its own on the context.
//
// The rule (written from PCL 1.8 segmentation/impl/extract_clusters.hpp; PCL is not linked, the checker is
// tests/cluster_reference.py): two different finite points are joined iff d2 < r2 (strict, as FLANN's radius set),
// r2 = (float) (tolerance * tolerance) with the product in double, d2 = g_d2's float form; the clusters are the
// connected components of that graph whose size lies in [max(min_cluster_size, 1), max_cluster_size], largest first,
// equal sizes by their smallest member index, the members of a cluster ascending.  A non-finite point is in no cluster.
//
// Launches of a call: pack + bounding box, the grid (count, scan, scatter), then
//   k_cluster_link     one lane per finite point, grid order: the radius walk of k_outlier_radius (wm_radius_walk.hpp);
//                      every hit at a SMALLER grid position joins the two trees of parent[] (a union-find over grid
//                      positions; see uf_find / uf_union for why no lane ever waits for another)
//   k_cluster_flatten  a launch of its own, so that every link is in: each point's root, and per root the smallest
//                      caller index (atomicMin) and the size (atomicAdd) -- integer atomics, order-independent
//   k_cluster_roots    the size rule and the counters; exclusive_scan + k_cluster_keys compact the kept roots
//   one fetch of the four counters, the sort of the kept roots by (0xFFFFFFFF - size) << 32 | smallest index,
//   k_cluster_rank + exclusive_scan (offsets), k_cluster_labels (caller order), and the stable sort of the points in
//   caller order by rank: the clusters' members back to back, ascending inside a cluster.
// A root is whatever grid position is the smallest of its component -- inside a cell that is the arrival order of the
// grid's atomics (see k_outlier_moments' note) -- so a root's number never reaches an output: the order of the
// clusters comes from (size, smallest caller index) alone.
#include <limits.h>
#include <string.h>  // (before rocPRIM's headers, which call memset)

#include "wm_radius_walk.hpp"
#include "wm_sort.hpp"

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

constexpr int kLinkBlock = 64;  // queries (threads) of a link workgroup: one wave, as k_outlier_radius

#define WM_UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ------------------------------------------------------------------ the union-find over grid positions
// Invariant: parent[x] <= x, and parent[x] is x (x is a root) or an ancestor of x in the forest -- at every moment and
// for every value parent[x] has EVER held, so a lane that reads an old value still holds an ancestor.  Two kinds of
// writes keep it: a root is hooked under a SMALLER root (compare-and-swap from its own number), and path halving
// replaces a non-root's parent by a smaller ancestor (atomicMin).  Parents only ever decrease.
//
// uf_find: every step moves to a strictly smaller position, so it ends after at most x steps whatever other lanes do.
// What it returns was a root when it was read; whether it still is, the caller's compare-and-swap decides.
__device__ __forceinline__ unsigned uf_find(unsigned *parent, unsigned x) {
    unsigned p = WM_UF_LOAD(parent + x);
    while (p != x) {
        const unsigned gp = WM_UF_LOAD(parent + p);
        if (gp != p) (void) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // halving
        x = p;
        p = gp;
    }
    return x;
}

// Join the trees of a and b.  Equal roots: one tree already (also when both reads were old: a common ancestor).
// Otherwise the larger root is hooked under the smaller by a compare-and-swap that succeeds only while it IS a root.
// A lost swap returns the parent somebody else gave it -- smaller than it -- and the join goes on from there: a + b
// strictly decreases from one round to the next, so the loop ends after a bounded number of rounds without ever
// waiting for another lane (a lost swap is another lane's progress: lock-free).
__device__ __forceinline__ void uf_union(unsigned *parent, unsigned a, unsigned b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
        unsigned expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = expected;  // hi's parent now: < hi
        b = lo;
    }
}

__global__ void __launch_bounds__(kBlock) k_cluster_init(unsigned *__restrict__ parent, unsigned n) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) parent[i] = i;
}

// One lane per finite point, grid order.  Each edge once: the hit at the smaller position is joined by the lane at the
// larger one (the lane itself, d2 = 0 at its own position, is no hit).  No cell-level shortcut: every pair is tested.
__global__ void __launch_bounds__(kLinkBlock)
    k_cluster_link(GridDev g, unsigned n, float r2, float r_cells, unsigned *parent) {
    __shared__ uint2 s_runs[kKnnRows * kLinkBlock];
    const unsigned i = blockIdx.x * kLinkBlock + threadIdx.x;
    if (i >= n) return;
    const float4 q = g.pts[i];
    radius_walk<false>(g, q, r_cells, s_runs, threadIdx.x, kLinkBlock, [&](unsigned j, const float4 &t) {
        if (j < i && g_d2(q.x, q.y, q.z, t) < r2) uf_union(parent, i, j);
        return false;
    });
}

// (behind the link launch: the forest is final, a find only shortens paths)
__global__ void __launch_bounds__(kBlock)
    k_cluster_flatten(const float4 *__restrict__ gpts, unsigned n, unsigned *parent, unsigned *__restrict__ root_of,
                      unsigned *min_idx, unsigned *size) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned r = uf_find(parent, i);
    const unsigned c = __float_as_uint(gpts[i].w);
    root_of[c] = r;
    atomicMin(&min_idx[r], c);
    atomicAdd(&size[r], 1u);
}

// res: [0] components, [1] kept clusters (k_cluster_keys), [2] points in kept clusters, [3] the largest kept cluster
__global__ void __launch_bounds__(kBlock)
    k_cluster_roots(const unsigned *__restrict__ size, unsigned n, unsigned lo, unsigned hi, unsigned *__restrict__ keep,
                    unsigned *res) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned s = i < n ? size[i] : 0u;
    const bool kept = s >= lo && s <= hi && s > 0u;
    if (i < n) keep[i] = kept ? 1u : 0u;
    unsigned roots = s > 0u ? 1u : 0u, pts = kept ? s : 0u, big = pts;
    for (int off = 32; off > 0; off >>= 1) {
        roots += __shfl_down(roots, off);
        pts += __shfl_down(pts, off);
        big = max(big, __shfl_down(big, off));
    }
    if ((threadIdx.x & 63) == 0 && roots) {
        atomicAdd(&res[0], roots);
        if (pts) atomicAdd(&res[2], pts);
        if (big) atomicMax(&res[3], big);
    }
}

// pos = the exclusive scan of keep (n + 1 entries): the kept roots' sort keys and numbers, compacted
__global__ void __launch_bounds__(kBlock)
    k_cluster_keys(const unsigned *__restrict__ keep, const unsigned *__restrict__ pos, const unsigned *__restrict__ size,
                   const unsigned *__restrict__ min_idx, unsigned n, unsigned long long *__restrict__ keys,
                   unsigned *__restrict__ vals, unsigned *__restrict__ res) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) res[1] = pos[n];
    if (i >= n || !keep[i]) return;
    keys[pos[i]] = ((unsigned long long) (0xFFFFFFFFu - size[i]) << 32) | min_idx[i];
    vals[pos[i]] = i;
}

// sorted[r] = the root of the cluster of rank r
__global__ void __launch_bounds__(kBlock)
    k_cluster_rank(const unsigned *__restrict__ sorted, const unsigned *__restrict__ size, unsigned m,
                   unsigned *__restrict__ rank_of, unsigned *__restrict__ size_by_rank) {
    const unsigned r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= m) return;
    const unsigned root = sorted[r];
    rank_of[root] = r;
    size_by_rank[r] = size[root];
}

// caller order: the label, and the pair (rank, index) of the member sort -- a point of no kept cluster gets key m and
// falls behind them all.  root_of[i] = kNoIdx: a non-finite point.
__global__ void __launch_bounds__(kBlock)
    k_cluster_labels(const unsigned *__restrict__ root_of, const unsigned *__restrict__ keep, const unsigned *__restrict__ rank_of,
                     unsigned n, unsigned m, int *__restrict__ labels, unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned root = root_of[i];
    int lab = WM_CLUSTER_NONE;
    if (root != kNoIdx) lab = keep[root] ? (int) rank_of[root] : WM_CLUSTER_REJECTED;
    if (labels) labels[i] = lab;
    if (keys) {
        keys[i] = lab >= 0 ? (unsigned) lab : m;
        vals[i] = i;
    }
}

// off = the exclusive scan of the sizes in rank order (m + 1 entries) -> the first `count` offsets, clamped to cap
__global__ void __launch_bounds__(kBlock)
    k_cluster_offsets(const unsigned *__restrict__ off, unsigned count, unsigned cap, unsigned *__restrict__ out) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    if (c < count) out[c] = min(off[c], cap);
}

}  // namespace

// The context's workspace of the cluster extraction: its own buffers, shared with nothing else on the context.
struct ClusterWs {
    DevBuf pts, parent, root_of, min_idx, size, keep, pos, rank_of, size_by_rank, off, labels, offsets, res;
    DevBuf keys_a, keys_b, vals_a, vals_b, sort_tmp;  // the two sorts' ping-pong pairs
    GridLevel grid;
    unsigned *h_res = nullptr;  // pinned: the four counters
};

void cluster_release(wm_ctx *ctx) {
    ClusterWs *w = static_cast<ClusterWs *>(ctx->cluster);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts, &w->parent, &w->root_of, &w->min_idx, &w->size, &w->keep, &w->pos, &w->rank_of,
                      &w->size_by_rank, &w->off, &w->labels, &w->offsets, &w->res, &w->keys_a, &w->keys_b, &w->vals_a,
                      &w->vals_b, &w->sort_tmp, &w->grid.pts, &w->grid.cell_start};
    for (DevBuf *b : bufs) b->release();
    if (w->h_res) (void) hipHostFree(w->h_res);
    delete w;
    ctx->cluster = nullptr;
}

namespace {

template <class K>
int cluster_sort(wm_ctx *ctx, ClusterWs &w, K *k_in, K *k_out, unsigned *v_in, unsigned *v_out, size_t n, unsigned bits) {
    size_t tmp_bytes = 0;
    WM_HIP(ctx, sort_pairs_low_bits((void *) nullptr, tmp_bytes, k_in, k_out, v_in, v_out, n, bits, ctx->stream,
                                    (size_t) ctx->tune_radix_min));
    WM_HIP(ctx, w.sort_tmp.reserve(tmp_bytes + 16));
    WM_HIP(ctx, sort_pairs_low_bits(w.sort_tmp.p, tmp_bytes, k_in, k_out, v_in, v_out, n, bits, ctx->stream,
                                    (size_t) ctx->tune_radix_min));
    return WM_OK;
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

}  // namespace

}  // namespace wm

using namespace wm;

extern "C" {

void wm_cluster_default_params(wm_cluster_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->tolerance = 0.0;  // extract_clusters.h: cluster_tolerance_ (0), min_pts_per_cluster_ (1), max_pts_per_cluster_ (max int)
    p->min_cluster_size = 1;
    p->max_cluster_size = INT_MAX;
}

int wm_cluster_extract(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_cluster_params *p,
                       int32_t *labels_out, int32_t *indices_out, size_t cap, uint32_t *offsets_out, size_t cap_clusters,
                       int out_mem, size_t *n_clusters, size_t *n_out, wm_cluster_stats *stats) {
    if (!ctx || !p || !n_out || !n_clusters || (n > 0 && !pts) || stride < 12 || (stride & 3) || n > 0x7FFFFFF0u ||
        (cap > 0 && !indices_out) || (cap_clusters > 0 && !offsets_out) || (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) ||
        (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE) || !std::isfinite(p->tolerance) || !(p->tolerance > 0) ||
        p->min_cluster_size < 0 || p->max_cluster_size < 0)
        return WM_ERR_ARG;
    *n_out = 0;
    *n_clusters = 0;
    if (stats) *stats = wm_cluster_stats{};
    const bool host_out = out_mem == WM_MEM_HOST;
    if (n == 0) {  // (no device is touched: offsets_out[0] can only be written where the host can write it)
        if (offsets_out && host_out) offsets_out[0] = 0;
        return WM_OK;
    }
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->cluster) ctx->cluster = new ClusterWs();
    ClusterWs &w = *static_cast<ClusterWs *>(ctx->cluster);
    if (!w.h_res) WM_HIP(ctx, hipHostMalloc((void **) &w.h_res, 4 * sizeof(unsigned), hipHostMallocDefault));
    hipStream_t st = ctx->stream;
    const unsigned nblocks = blocks_of(n);

    // the outputs' places: the caller's own in device memory, else the workspace's
    WM_HIP(ctx, w.pts.reserve(n * sizeof(float4)));
    WM_HIP(ctx, w.root_of.reserve(n * 4));
    WM_HIP(ctx, w.res.reserve(4 * sizeof(unsigned)));
    int *d_labels = nullptr;
    if (labels_out) {
        if (host_out) WM_HIP(ctx, w.labels.reserve(n * 4));
        d_labels = host_out ? w.labels.as<int>() : labels_out;
    }
    unsigned *d_offsets = nullptr;
    if (offsets_out) {
        if (host_out) WM_HIP(ctx, w.offsets.reserve(4));
        d_offsets = host_out ? w.offsets.as<unsigned>() : offsets_out;
    }

    if (stats) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, w.pts.as<float4>()));
    Bbox bb;
    size_t n_finite = 0;
    WM_TRY(compute_bbox(ctx, w.pts.as<float4>(), n, &bb, &n_finite));
    if (stats) stats->n_finite = n_finite;
    if (n_finite == 0) {  // every label NONE (-1: all bits set), no cluster
        if (labels_out) WM_HIP(ctx, hipMemsetAsync(d_labels, 0xFF, n * 4, st));
        if (offsets_out) WM_HIP(ctx, hipMemsetAsync(d_offsets, 0, 4, st));
        WM_HIP(ctx, hipStreamSynchronize(st));
        if (host_out) {
            if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, n * 4, hipMemcpyDeviceToHost));
            if (offsets_out) offsets_out[0] = 0;
        }
        return WM_OK;
    }

    const float r2 = (float) (p->tolerance * p->tolerance);
    const float rf = sqrtf(r2) * 1.0001f;  // (a point with float d2 < r2 lies within this of the query)
    WM_TRY(build_call_grid(ctx, w.pts.as<float4>(), n, n_finite, bb,
                           fminf((float) p->tolerance, 1.0e30f) / ctx->tune_cluster_cell_div, &w.grid));
    const GridDev &g = w.grid.d;
    const unsigned nf = (unsigned) n_finite, fblocks = blocks_of(n_finite);

    WM_HIP(ctx, w.parent.reserve(n_finite * 4));
    WM_HIP(ctx, w.min_idx.reserve(n_finite * 4));
    WM_HIP(ctx, w.size.reserve(n_finite * 4));
    WM_HIP(ctx, w.keep.reserve(n_finite * 4));
    WM_HIP(ctx, w.pos.reserve((n_finite + 1) * 4));
    WM_HIP(ctx, w.rank_of.reserve(n_finite * 4));
    WM_HIP(ctx, w.size_by_rank.reserve(n_finite * 4));
    WM_HIP(ctx, w.off.reserve((n_finite + 1) * 4));
    WM_HIP(ctx, w.keys_a.reserve(n * 8));
    WM_HIP(ctx, w.keys_b.reserve(n * 8));
    WM_HIP(ctx, w.vals_a.reserve(n * 4));
    WM_HIP(ctx, w.vals_b.reserve(n * 4));
    unsigned *parent = w.parent.as<unsigned>(), *root_of = w.root_of.as<unsigned>(), *min_idx = w.min_idx.as<unsigned>();
    unsigned *size = w.size.as<unsigned>(), *keep = w.keep.as<unsigned>(), *pos = w.pos.as<unsigned>();
    unsigned *res = w.res.as<unsigned>();

    WM_HIP(ctx, hipMemsetAsync(root_of, 0xFF, n * 4, st));         // kNoIdx
    WM_HIP(ctx, hipMemsetAsync(min_idx, 0xFF, n_finite * 4, st));
    WM_HIP(ctx, hipMemsetAsync(size, 0, n_finite * 4, st));
    WM_HIP(ctx, hipMemsetAsync(res, 0, 4 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_cluster_init, dim3(fblocks), dim3(kBlock), 0, st, parent, nf);
    hipLaunchKernelGGL(k_cluster_link, dim3((unsigned) ((n_finite + kLinkBlock - 1) / kLinkBlock)), dim3(kLinkBlock), 0, st,
                       g, nf, r2, rf * g.inv_h, parent);
    hipLaunchKernelGGL(k_cluster_flatten, dim3(fblocks), dim3(kBlock), 0, st, g.pts, nf, parent, root_of, min_idx, size);
    const unsigned lo = (unsigned) std::max(p->min_cluster_size, 1), hi = (unsigned) p->max_cluster_size;
    hipLaunchKernelGGL(k_cluster_roots, dim3(fblocks), dim3(kBlock), 0, st, (const unsigned *) size, nf, lo, hi, keep, res);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, keep, n_finite, pos));
    hipLaunchKernelGGL(k_cluster_keys, dim3(fblocks), dim3(kBlock), 0, st, (const unsigned *) keep, (const unsigned *) pos,
                       (const unsigned *) size, (const unsigned *) min_idx, nf, w.keys_a.as<unsigned long long>(),
                       w.vals_a.as<unsigned>(), res);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(fast_fetch(ctx, w.h_res, res, 4 * sizeof(unsigned)));
    const size_t n_comp = w.h_res[0], m = w.h_res[1], kept = w.h_res[2], largest = w.h_res[3];

    const unsigned *sorted_pts = nullptr;
    if (m > 0) {
        WM_TRY(cluster_sort(ctx, w, w.keys_a.as<unsigned long long>(), w.keys_b.as<unsigned long long>(),
                            w.vals_a.as<unsigned>(), w.vals_b.as<unsigned>(), m, 64u));
        hipLaunchKernelGGL(k_cluster_rank, dim3(blocks_of(m)), dim3(kBlock), 0, st, (const unsigned *) w.vals_b.as<unsigned>(),
                           (const unsigned *) size, (unsigned) m, w.rank_of.as<unsigned>(), w.size_by_rank.as<unsigned>());
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(exclusive_scan(ctx, w.size_by_rank.as<unsigned>(), m, w.off.as<unsigned>()));
    } else {
        WM_HIP(ctx, hipMemsetAsync(w.off.p, 0, 4, st));
    }
    hipLaunchKernelGGL(k_cluster_labels, dim3(nblocks), dim3(kBlock), 0, st, (const unsigned *) root_of, (const unsigned *) keep,
                       (const unsigned *) w.rank_of.as<unsigned>(), (unsigned) n, (unsigned) m, d_labels,
                       m > 0 ? w.keys_a.as<unsigned>() : (unsigned *) nullptr, w.vals_a.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    if (m > 0) {
        unsigned bits = 0;
        while (((size_t) 1 << bits) <= m) ++bits;  // the keys are 0 ... m
        WM_TRY(cluster_sort(ctx, w, w.keys_a.as<unsigned>(), w.keys_b.as<unsigned>(), w.vals_a.as<unsigned>(),
                            w.vals_b.as<unsigned>(), n, bits));
        sorted_pts = w.vals_b.as<unsigned>();
    }
    const size_t n_idx = std::min(kept, cap), n_off = std::min(m, cap_clusters) + 1;
    if (offsets_out) {
        if (host_out) {
            WM_HIP(ctx, w.offsets.reserve(n_off * 4));
            d_offsets = w.offsets.as<unsigned>();
        }
        hipLaunchKernelGGL(k_cluster_offsets, dim3(blocks_of(n_off)), dim3(kBlock), 0, st, (const unsigned *) w.off.as<unsigned>(),
                           (unsigned) n_off, (unsigned) std::min(cap, (size_t) 0xFFFFFFFFu), d_offsets);
        WM_HIP(ctx, hipGetLastError());
    }
    if (!host_out && n_idx)
        WM_HIP(ctx, hipMemcpyAsync(indices_out, sorted_pts, n_idx * 4, hipMemcpyDeviceToDevice, st));
    if (stats) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipStreamSynchronize(st));

    *n_out = kept;
    *n_clusters = m;
    if (stats) {
        stats->n_components = n_comp;
        stats->n_clusters = m;
        stats->n_clustered = kept;
        stats->largest = largest;
        (void) hipEventElapsedTime(&stats->kernel_ms, ctx->ev_a, ctx->ev_b);
    }
    if (host_out) {
        if (n_idx) WM_HIP(ctx, hipMemcpy(indices_out, sorted_pts, n_idx * 4, hipMemcpyDeviceToHost));
        if (offsets_out) WM_HIP(ctx, hipMemcpy(offsets_out, d_offsets, n_off * 4, hipMemcpyDeviceToHost));
        if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, n * 4, hipMemcpyDeviceToHost));
    }
    return kept > cap || m > cap_clusters ? WM_ERR_ARG : WM_OK;
}

}  // extern "C"
