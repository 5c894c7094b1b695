// wm_cluster.hip -- Euclidean cluster extraction on the device: pcl::EuclideanClusterExtraction as one cloud-in /
// clusters-out call (wm_cluster_extract), shaped like wm_outlier_filter: the call packs the cloud, builds a cell-sorted
// grid over it for this call alone, and works in a workspace of its own on the context.  wm_cluster_extract_batch is
// the same for a queue of scans: one set of kernels with a scan dimension, as wm_ground_segment_batch.
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
//
// wm_cluster_extract_cond (pcl::ConditionalEuclideanClustering with a normal and / or scalar test on every edge; the
// checker is tests/cluster_cond_reference.py) is the single call with two launches in place of the link's one:
// k_cluster_attr brings the caller's four floats per point into the grid's order, and k_cluster_link<true> asks them
// about every pair that passes the distance test before it joins the pair.  Both tests are symmetric in their two
// points, so the clusters are still the connected components of an undirected graph and nothing behind the link
// changes.  flags == 0 launches k_cluster_link<false>, which is the kernel wm_cluster_extract launches.
//
// A batch (ClScan: a scan's row of the device table; tab == nullptr is the single call, its scan handed over by
// value): its front -- the table, the packed batch positions, a lattice per scan inside ONE cell-sorted array of grid
// positions -- is wm_scan_batch.hpp's, shared with wm_outlier_filter_batch.  A scan's GridDev points at its own slice
// of cell_start and at the shared array, so a walk never meets a point of another scan, and the union-find, the
// counters, the two sorts and the outputs run over the whole batch at once: the sort key of a kept root leads with its
// scan, a member's with its cluster's batch-wide rank.  The number of launches and host waits does not depend on the
// number of scans.
#include <limits.h>
#include <string.h>  // (before rocPRIM's headers, which call memset)

#include "wm_radius_walk.hpp"
#include "wm_scan_batch.hpp"
#include "wm_sort.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

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
// A batch: a workgroup (one wave) belongs to one scan, found from the table of first workgroups, so the scan's
// lattice is the same for every lane (scalar registers) and its runs hold the scan's own points only; the positions
// it joins are the batch's.
//
// COND (wm_cluster_extract_cond with flags != 0): an edge that passes the distance test must also pass the enabled
// tests on the two points' attributes, attr_g (grid order, written by k_cluster_attr in an earlier launch on the
// stream: plain loads).  The lane's own record is loaded once; the candidate's only behind j < i and d2 < r2, so a
// candidate that fails the distance test costs no attribute traffic.  Both tests are symmetric in their two points bit
// for bit (products and sums commute, fabsf(a - b) == fabsf(b - a)), and a NaN on either side fails the comparison.
struct LinkCond {
    const float4 *attr_g;
    int flags;               // WM_CLUSTER_COND_*
    float cos_min, max_diff;  // (float) cos(max_normal_angle), (float) max_scalar_diff
};

__device__ __forceinline__ bool cond_holds(const LinkCond &c, const float4 &a, const float4 &b) {
    const float dot = __fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z));
    const bool normal = !(c.flags & WM_CLUSTER_COND_NORMAL) || fabsf(dot) >= c.cos_min;
    const bool scalar = !(c.flags & WM_CLUSTER_COND_SCALAR) || fabsf(__fsub_rn(a.w, b.w)) <= c.max_diff;
    return normal && scalar;
}

template <bool COND>
__global__ void __launch_bounds__(kLinkBlock)
    k_cluster_link(GridDev g, const ClScan *__restrict__ tab, unsigned S, unsigned n, float r2, float rf, unsigned *parent,
                   LinkCond cond) {
    __shared__ uint2 s_runs[kKnnRows * kLinkBlock];
    unsigned i = blockIdx.x * kLinkBlock + threadIdx.x;
    if (tab) {
        const unsigned k = cl_find(tab, S, blockIdx.x, [](const ClScan &s) { return s.lblk0; });
        g = tab[k].g;
        i = tab[k].g0 + (blockIdx.x - tab[k].lblk0) * kLinkBlock + threadIdx.x;
        n = tab[k].g0 + tab[k].nf;
    }
    if (i >= n) return;
    const float4 q = g.pts[i];
    float4 own = make_float4(0.f, 0.f, 0.f, 0.f);
    if (COND) own = cond.attr_g[i];
    radius_walk<false>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kLinkBlock, [&](unsigned j, const float4 &t) {
        if (j < i && g_d2(q.x, q.y, q.z, t) < r2) {
            if (!COND || cond_holds(cond, own, cond.attr_g[j])) uf_union(parent, i, j);
        }
        return false;
    });
}

// One lane per grid position: the caller's four floats (record pts[i].w of `raw`, attr_stride bytes each) into the
// grid's order, so that the link kernel's attribute reads have the locality its point reads have.
__global__ void __launch_bounds__(kBlock)
    k_cluster_attr(const float4 *__restrict__ gpts, unsigned n, const unsigned char *__restrict__ raw, size_t attr_stride,
                   float4 *__restrict__ attr_g) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *a = reinterpret_cast<const float *>(raw + (size_t) __float_as_uint(gpts[i].w) * attr_stride);
    attr_g[i] = make_float4(a[0], a[1], a[2], a[3]);
}

// (behind the link launch: the forest is final, a find only shortens paths)  c: the point's batch position
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

// res, four per scan: [0] components, [1] kept clusters (k_cluster_keys), [2] points in kept clusters, [3] the largest
// kept cluster.  A wave whose 64 grid positions are of one scan adds its sums once; a wave across a scan boundary adds
// root by root.
__global__ void __launch_bounds__(kBlock)
    k_cluster_roots(const unsigned *__restrict__ size, unsigned n, unsigned lo, unsigned hi, unsigned *__restrict__ keep,
                    unsigned *res, const ClScan *__restrict__ tab, unsigned S) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned s = i < n ? size[i] : 0u;
    const bool kept = s >= lo && s <= hi && s > 0u;
    if (i < n) keep[i] = kept ? 1u : 0u;
    unsigned roots = s > 0u ? 1u : 0u, pts = kept ? s : 0u, big = pts;
    if (tab) {
        const unsigned w0 = i & ~63u;
        if (w0 >= n) return;  // (the whole wave)
        const unsigned k0 = cl_by_grid(tab, S, w0), k1 = cl_by_grid(tab, S, min(w0 + 63u, n - 1u));
        if (k0 != k1) {
            if (roots) {
                unsigned *r = res + 4u * cl_by_grid(tab, S, i);
                atomicAdd(&r[0], 1u);
                if (pts) {
                    atomicAdd(&r[2], pts);
                    atomicMax(&r[3], big);
                }
            }
            return;
        }
        res += 4u * k0;
    }
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

// pos = the exclusive scan of keep (n + 1 entries): the kept roots' sort keys and numbers, compacted.  The key, most
// significant first: the scan, (2^b - 1) - size, the smallest member's index in its scan -- fields of b bits (b = 32
// and no scan field for the single call).  The grid positions are scan-major, so scan k's kept roots are pos's
// increase over its positions.
__global__ void __launch_bounds__(kBlock)
    k_cluster_keys(const unsigned *__restrict__ keep, const unsigned *__restrict__ pos, const unsigned *__restrict__ size,
                   const unsigned *__restrict__ min_idx, unsigned n, unsigned long long *__restrict__ keys,
                   unsigned *__restrict__ vals, unsigned *__restrict__ res, const ClScan *__restrict__ tab, unsigned S,
                   unsigned b) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (!tab) {
        if (i == 0) res[1] = pos[n];
    } else if (i < S) {
        res[4u * i + 1u] = pos[tab[i].g0 + tab[i].nf] - pos[tab[i].g0];
    }
    if (i >= n || !keep[i]) return;
    unsigned long long key;
    if (tab) {
        const unsigned k = cl_by_grid(tab, S, i);
        key = ((unsigned long long) k << (2u * b)) | ((unsigned long long) (((1u << b) - 1u) - size[i]) << b) |
              (min_idx[i] - tab[k].off);
    } else {
        key = ((unsigned long long) (0xFFFFFFFFu - size[i]) << 32) | min_idx[i];
    }
    keys[pos[i]] = key;
    vals[pos[i]] = i;
}

// sorted[r] = the root of the cluster of rank r (batch-wide); lrank_of: its rank inside its scan, the label
__global__ void __launch_bounds__(kBlock)
    k_cluster_rank(const unsigned *__restrict__ sorted, const unsigned *__restrict__ size, unsigned m,
                   unsigned *__restrict__ rank_of, unsigned *__restrict__ size_by_rank, const ClScan *__restrict__ tab,
                   unsigned S, const unsigned *__restrict__ pos, unsigned *__restrict__ lrank_of) {
    const unsigned r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= m) return;
    const unsigned root = sorted[r];
    rank_of[root] = r;
    size_by_rank[r] = size[root];
    if (tab) lrank_of[root] = r - pos[tab[cl_by_grid(tab, S, root)].g0];
}

// caller order: the label, and the pair (rank, position) of the member sort -- a point of no kept cluster gets key m
// and falls behind them all.  root_of[i] = kNoIdx: a non-finite point.
__global__ void __launch_bounds__(kBlock)
    k_cluster_labels(const unsigned *__restrict__ root_of, const unsigned *__restrict__ keep, const unsigned *__restrict__ rank_of,
                     const unsigned *__restrict__ lrank_of, unsigned n, unsigned m, int *__restrict__ labels,
                     unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned root = root_of[i];
    const bool in = root != kNoIdx && keep[root];
    if (labels) labels[i] = in ? (int) lrank_of[root] : root != kNoIdx ? WM_CLUSTER_REJECTED : WM_CLUSTER_NONE;
    if (keys) {
        keys[i] = in ? rank_of[root] : m;
        vals[i] = i;
    }
}

// off = the exclusive scan of the sizes in rank order (m + 1 entries) -> the first `count` offsets, clamped to cap
__global__ void __launch_bounds__(kBlock)
    k_cluster_offsets(const unsigned *__restrict__ off, unsigned count, unsigned cap, unsigned *__restrict__ out) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    if (c < count) out[c] = min(off[c], cap);
}

// The sorted member list (batch positions) -> the index inside the member's scan and, for points_out, its x y z as the
// packed cloud holds them (a member is finite, and a finite point is packed bit for bit): cl_write_record.
__global__ void __launch_bounds__(kBlock)
    k_cluster_emit(const unsigned *__restrict__ sorted, unsigned count, const ClScan *__restrict__ tab, unsigned S,
                   const float4 *__restrict__ pts, int *__restrict__ idx_out, unsigned char *__restrict__ pout,
                   size_t out_stride) {
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= count) return;
    const unsigned p = sorted[j];
    if (idx_out) idx_out[j] = (int) (tab ? p - tab[cl_by_point(tab, S, p)].off : p);
    if (pout) cl_write_record(pout, j, out_stride, pts[p]);
}

}  // namespace

// The context's workspace of the cluster extraction: its own buffers, shared with nothing else on the context.
struct ClusterWs {
    DevBuf parent, root_of, min_idx, size, keep, pos, rank_of, lrank_of, size_by_rank, off, labels, offsets, res;
    DevBuf keys_a, keys_b, vals_a, vals_b, sort_tmp;  // the two sorts' ping-pong pairs
    DevBuf idx, pout;                                 // host outputs on their way
    DevBuf attr_raw, attr_g;  // wm_cluster_extract_cond: host attributes uploaded, and the four floats in grid order
    ScanBatchBufs sb;  // the packed cloud and its grid; a batch's front (wm_scan_batch.hpp)
    PinnedBuf h_res;   // the counters, four per scan
};

void cluster_release(wm_ctx *ctx) {
    ClusterWs *w = static_cast<ClusterWs *>(ctx->cluster);
    if (!w) return;
    DevBuf *bufs[] = {&w->parent, &w->root_of, &w->min_idx, &w->size, &w->keep, &w->pos, &w->rank_of,
                      &w->lrank_of, &w->size_by_rank, &w->off, &w->labels, &w->offsets, &w->res, &w->keys_a, &w->keys_b,
                      &w->vals_a, &w->vals_b, &w->sort_tmp, &w->idx, &w->pout, &w->attr_raw, &w->attr_g};
    for (DevBuf *b : bufs) b->release();
    w->sb.release();
    w->h_res.release();
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

unsigned bits_of(unsigned long long v) {  // the bits that hold 0 ... v
    unsigned b = 0;
    while (b < 64 && (v >> b) != 0ull) ++b;
    return b;
}

bool cl_args_ok(const wm_cluster_params *p, size_t stride, int mem, int out_mem) {
    return p && stride >= 12 && !(stride & 3) && (mem == WM_MEM_HOST || mem == WM_MEM_DEVICE) &&
           (out_mem == WM_MEM_HOST || out_mem == WM_MEM_DEVICE) && std::isfinite(p->tolerance) && p->tolerance > 0 &&
           p->min_cluster_size >= 0 && p->max_cluster_size >= 0;
}

// What the front of a call (one scan or a batch) hands to the kernels behind the grid, and where the results go.
struct ClCall {
    const ClScan *tab = nullptr;  // nullptr: one scan, its grid in `g`
    unsigned S = 1;
    GridDev g{};
    size_t n = 0, nf = 0;  // the call's points (batch positions) and the finite ones (grid positions)
    unsigned link_blocks = 0, field_bits = 32;
    const wm_cluster_params *p = nullptr;
    bool host_out = true, timed = false;
    int32_t *labels_out = nullptr, *indices_out = nullptr;
    size_t cap = 0;
    void *points_out = nullptr;
    size_t out_stride = 0;
    uint32_t *offsets_out = nullptr;
    size_t cap_clusters = 0;
    LinkCond cond{};                          // flags != 0: wm_cluster_extract_cond's edge tests (attr_g set by cl_back)
    const unsigned char *attr_raw = nullptr;  // the caller's attribute records in device memory
    size_t attr_stride = 0;
    size_t m = 0, kept = 0;  // results: the kept clusters and their points; the counters are in w.h_res
    float ms = 0.f;
};

// The device places of the outputs: the caller's own in device memory, else the workspace's.
int cl_labels_place(wm_ctx *ctx, ClusterWs &w, const ClCall &c, int **d_labels) {
    *d_labels = nullptr;
    if (!c.labels_out) return WM_OK;
    if (c.host_out) WM_HIP(ctx, w.labels.reserve(c.n * 4));
    *d_labels = c.host_out ? w.labels.as<int>() : c.labels_out;
    return WM_OK;
}

// A call without a finite point: every label NONE (-1: all bits set), no cluster.
int cl_nothing_finite(wm_ctx *ctx, ClusterWs &w, const ClCall &c) {
    hipStream_t st = ctx->stream;
    int *d_labels = nullptr;
    WM_TRY(cl_labels_place(ctx, w, c, &d_labels));
    if (c.labels_out) WM_HIP(ctx, hipMemsetAsync(d_labels, 0xFF, c.n * 4, st));
    if (c.offsets_out && !c.host_out) WM_HIP(ctx, hipMemsetAsync(c.offsets_out, 0, 4, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (c.host_out) {
        if (c.labels_out) WM_HIP(ctx, hipMemcpy(c.labels_out, d_labels, c.n * 4, hipMemcpyDeviceToHost));
        if (c.offsets_out) c.offsets_out[0] = 0;
    }
    return WM_OK;
}

// Behind the grid: link, flatten, the size rule, the two sorts, the outputs.  One fetch (the counters of all scans) and
// the wait at the end.  The single call: 4 memsets, 13 launches and the two sorts; a batch: one launch more
// (k_cluster_emit) -- whatever the number of scans.
int cl_back(wm_ctx *ctx, ClusterWs &w, ClCall &c) {
    hipStream_t st = ctx->stream;
    const size_t n = c.n, n_finite = c.nf;
    const unsigned nf = (unsigned) n_finite, fblocks = blocks_of(n_finite), S = c.S;
    const ClScan *tab = c.tab;
    const float r2 = (float) (c.p->tolerance * c.p->tolerance);
    const float rf = sqrtf(r2) * 1.0001f;  // (a point with float d2 < r2 lies within this of the query)
    const GridDev &g = c.g;                // (a batch: only its pts, the shared array, is read from here)

    int *d_labels = nullptr;
    WM_TRY(cl_labels_place(ctx, w, c, &d_labels));
    WM_HIP(ctx, w.root_of.reserve(n * 4));
    WM_HIP(ctx, w.res.reserve((size_t) S * 4 * sizeof(unsigned)));
    WM_HIP(ctx, w.h_res.reserve((size_t) S * 4 * sizeof(unsigned)));
    WM_HIP(ctx, w.parent.reserve(n_finite * 4));
    WM_HIP(ctx, w.min_idx.reserve(n_finite * 4));
    WM_HIP(ctx, w.size.reserve(n_finite * 4));
    WM_HIP(ctx, w.keep.reserve(n_finite * 4));
    WM_HIP(ctx, w.pos.reserve((n_finite + 1) * 4));
    WM_HIP(ctx, w.rank_of.reserve(n_finite * 4));
    if (tab) WM_HIP(ctx, w.lrank_of.reserve(n_finite * 4));
    WM_HIP(ctx, w.size_by_rank.reserve(n_finite * 4));
    WM_HIP(ctx, w.off.reserve((n_finite + 1) * 4));
    WM_HIP(ctx, w.keys_a.reserve(n * 8));
    WM_HIP(ctx, w.keys_b.reserve(n * 8));
    WM_HIP(ctx, w.vals_a.reserve(n * 4));
    WM_HIP(ctx, w.vals_b.reserve(n * 4));
    unsigned *parent = w.parent.as<unsigned>(), *root_of = w.root_of.as<unsigned>(), *min_idx = w.min_idx.as<unsigned>();
    unsigned *size = w.size.as<unsigned>(), *keep = w.keep.as<unsigned>(), *pos = w.pos.as<unsigned>();
    unsigned *res = w.res.as<unsigned>(), *rank_of = w.rank_of.as<unsigned>();
    unsigned *lrank_of = tab ? w.lrank_of.as<unsigned>() : rank_of;
    unsigned *h_res = w.h_res.as<unsigned>();

    WM_HIP(ctx, hipMemsetAsync(root_of, 0xFF, n * 4, st));         // kNoIdx
    WM_HIP(ctx, hipMemsetAsync(min_idx, 0xFF, n_finite * 4, st));
    WM_HIP(ctx, hipMemsetAsync(size, 0, n_finite * 4, st));
    WM_HIP(ctx, hipMemsetAsync(res, 0, (size_t) S * 4 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_cluster_init, dim3(fblocks), dim3(kBlock), 0, st, parent, nf);
    if (c.cond.flags) {  // two launches in place of one: the attributes into grid order, the link with its edge tests
        WM_HIP(ctx, w.attr_g.reserve(n_finite * sizeof(float4)));
        c.cond.attr_g = w.attr_g.as<float4>();
        hipLaunchKernelGGL(k_cluster_attr, dim3(fblocks), dim3(kBlock), 0, st, g.pts, nf, c.attr_raw, c.attr_stride,
                           w.attr_g.as<float4>());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cluster_link<true>), dim3(c.link_blocks), dim3(kLinkBlock), 0, st, g, tab, S, nf, r2,
                           rf, parent, c.cond);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cluster_link<false>), dim3(c.link_blocks), dim3(kLinkBlock), 0, st, g, tab, S, nf, r2,
                           rf, parent, LinkCond{});
    }
    hipLaunchKernelGGL(k_cluster_flatten, dim3(fblocks), dim3(kBlock), 0, st, g.pts, nf, parent, root_of, min_idx, size);
    const unsigned lo = (unsigned) std::max(c.p->min_cluster_size, 1), hi = (unsigned) c.p->max_cluster_size;
    hipLaunchKernelGGL(k_cluster_roots, dim3(fblocks), dim3(kBlock), 0, st, (const unsigned *) size, nf, lo, hi, keep, res,
                       tab, S);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, keep, n_finite, pos));
    hipLaunchKernelGGL(k_cluster_keys, dim3(blocks_of(std::max(n_finite, tab ? (size_t) S : (size_t) 0))), dim3(kBlock), 0, st,
                       (const unsigned *) keep, (const unsigned *) pos, (const unsigned *) size, (const unsigned *) min_idx, nf,
                       w.keys_a.as<unsigned long long>(), w.vals_a.as<unsigned>(), res, tab, S, c.field_bits);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(fast_fetch(ctx, h_res, res, (size_t) S * 4 * sizeof(unsigned)));
    size_t m = 0, kept = 0;
    for (unsigned k = 0; k < S; ++k) {
        m += h_res[4 * k + 1];
        kept += h_res[4 * k + 2];
    }

    const unsigned *sorted_pts = nullptr;
    if (m > 0) {
        const unsigned key_bits = tab ? bits_of(S - 1u) + 2u * c.field_bits : 64u;
        WM_TRY(cluster_sort(ctx, w, w.keys_a.as<unsigned long long>(), w.keys_b.as<unsigned long long>(),
                            w.vals_a.as<unsigned>(), w.vals_b.as<unsigned>(), m, std::max(key_bits, 1u)));
        hipLaunchKernelGGL(k_cluster_rank, dim3(blocks_of(m)), dim3(kBlock), 0, st, (const unsigned *) w.vals_b.as<unsigned>(),
                           (const unsigned *) size, (unsigned) m, rank_of, w.size_by_rank.as<unsigned>(), tab, S,
                           (const unsigned *) pos, lrank_of);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(exclusive_scan(ctx, w.size_by_rank.as<unsigned>(), m, w.off.as<unsigned>()));
    } else {
        WM_HIP(ctx, hipMemsetAsync(w.off.p, 0, 4, st));
    }
    hipLaunchKernelGGL(k_cluster_labels, dim3(blocks_of(n)), dim3(kBlock), 0, st, (const unsigned *) root_of, (const unsigned *) keep,
                       (const unsigned *) rank_of, (const unsigned *) lrank_of, (unsigned) n, (unsigned) m, d_labels,
                       m > 0 ? w.keys_a.as<unsigned>() : (unsigned *) nullptr, w.vals_a.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    if (m > 0) {
        unsigned bits = 0;
        while (((size_t) 1 << bits) <= m) ++bits;  // the keys are 0 ... m
        WM_TRY(cluster_sort(ctx, w, w.keys_a.as<unsigned>(), w.keys_b.as<unsigned>(), w.vals_a.as<unsigned>(),
                            w.vals_b.as<unsigned>(), n, bits));
        sorted_pts = w.vals_b.as<unsigned>();
    }
    const size_t n_idx = std::min(kept, c.cap), n_off = std::min(m, c.cap_clusters) + 1;
    unsigned *d_offsets = nullptr;
    if (c.offsets_out) {
        d_offsets = c.offsets_out;
        if (c.host_out) {
            WM_HIP(ctx, w.offsets.reserve(n_off * 4));
            d_offsets = w.offsets.as<unsigned>();
        }
        hipLaunchKernelGGL(k_cluster_offsets, dim3(blocks_of(n_off)), dim3(kBlock), 0, st, (const unsigned *) w.off.as<unsigned>(),
                           (unsigned) n_off, (unsigned) std::min(c.cap, (size_t) 0xFFFFFFFFu), d_offsets);
        WM_HIP(ctx, hipGetLastError());
    }
    // the members: the sorted list itself for one scan without points_out, else through k_cluster_emit
    const bool emit = n_idx && (tab || c.points_out);
    const int *d_idx = reinterpret_cast<const int *>(sorted_pts);
    unsigned char *d_pout = static_cast<unsigned char *>(c.points_out);
    if (emit) {
        int *idx = c.indices_out;
        if (c.host_out) {
            WM_HIP(ctx, w.idx.reserve(n_idx * 4));
            idx = w.idx.as<int>();
            if (c.points_out) {
                WM_HIP(ctx, w.pout.reserve(n_idx * c.out_stride));
                d_pout = w.pout.as<unsigned char>();
            }
        }
        hipLaunchKernelGGL(k_cluster_emit, dim3(blocks_of(n_idx)), dim3(kBlock), 0, st, sorted_pts, (unsigned) n_idx, tab, S,
                           (const float4 *) w.sb.pts.as<float4>(), idx, d_pout, c.out_stride);
        WM_HIP(ctx, hipGetLastError());
        d_idx = idx;
    } else if (!c.host_out && n_idx) {
        WM_HIP(ctx, hipMemcpyAsync(c.indices_out, sorted_pts, n_idx * 4, hipMemcpyDeviceToDevice, st));
    }
    if (c.timed) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (c.timed) (void) hipEventElapsedTime(&c.ms, ctx->ev_a, ctx->ev_b);
    c.m = m;
    c.kept = kept;
    if (c.host_out) {
        if (n_idx) WM_HIP(ctx, hipMemcpy(c.indices_out, d_idx, n_idx * 4, hipMemcpyDeviceToHost));
        if (n_idx && c.points_out) WM_HIP(ctx, hipMemcpy(c.points_out, d_pout, n_idx * c.out_stride, hipMemcpyDeviceToHost));
        if (c.offsets_out) WM_HIP(ctx, hipMemcpy(c.offsets_out, d_offsets, n_off * 4, hipMemcpyDeviceToHost));
        if (c.labels_out) WM_HIP(ctx, hipMemcpy(c.labels_out, d_labels, n * 4, hipMemcpyDeviceToHost));
    }
    return kept > c.cap || m > c.cap_clusters ? WM_ERR_ARG : WM_OK;
}

void cl_stats_out(const unsigned *h, size_t n_finite, float ms, wm_cluster_stats *s) {
    s->n_finite = n_finite;
    s->n_components = h[0];
    s->n_clusters = h[1];
    s->n_clustered = h[2];
    s->largest = h[3];
    s->kernel_ms = ms;
}

// One scan, handed to the kernels by value: no table, no staging.  This is wm_cluster_extract, and
// wm_cluster_extract_batch for a batch of one (arguments checked by the callers; the outputs zeroed).
int cl_one(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_cluster_params *p, int32_t *labels_out,
           int32_t *indices_out, size_t cap, void *points_out, size_t out_stride, uint32_t *offsets_out, size_t cap_clusters,
           int out_mem, size_t *n_clusters, size_t *n_out, wm_cluster_stats *stats, float *kernel_ms,
           const LinkCond *cond = nullptr, const void *attr = nullptr, size_t attr_stride = 0, int attr_mem = WM_MEM_HOST) {
    ClCall c;
    c.host_out = out_mem == WM_MEM_HOST;
    if (n == 0) {  // (no device is touched: offsets_out[0] can only be written where the host can write it)
        if (offsets_out && c.host_out) offsets_out[0] = 0;
        return WM_OK;
    }
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->cluster) ctx->cluster = new ClusterWs();
    ClusterWs &w = *static_cast<ClusterWs *>(ctx->cluster);
    hipStream_t st = ctx->stream;
    c.n = n;
    c.p = p;
    c.timed = stats || kernel_ms;
    c.labels_out = labels_out;
    c.indices_out = indices_out;
    c.cap = cap;
    c.points_out = points_out;
    c.out_stride = points_out ? out_stride : 0;
    c.offsets_out = offsets_out;
    c.cap_clusters = cap_clusters;

    if (cond && cond->flags) {
        c.cond = *cond;
        c.attr_stride = attr_stride;
        c.attr_raw = static_cast<const unsigned char *>(attr);
        if (attr_mem == WM_MEM_HOST) {  // uploaded first, as a host cloud is (pageable memory: a blocking copy)
            WM_HIP(ctx, hipStreamSynchronize(st));
            WM_HIP(ctx, w.attr_raw.reserve(n * attr_stride));
            WM_HIP(ctx, hipMemcpy(w.attr_raw.p, attr, n * attr_stride, hipMemcpyHostToDevice));
            c.attr_raw = w.attr_raw.as<unsigned char>();
        }
    }
    WM_HIP(ctx, w.sb.pts.reserve(n * sizeof(float4)));
    if (c.timed) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, w.sb.pts.as<float4>()));
    Bbox bb;
    size_t n_finite = 0;
    WM_TRY(compute_bbox(ctx, w.sb.pts.as<float4>(), n, &bb, &n_finite));
    if (stats) stats->n_finite = n_finite;
    if (n_finite == 0) return cl_nothing_finite(ctx, w, c);
    WM_TRY(build_call_grid(ctx, w.sb.pts.as<float4>(), n, n_finite, bb,
                           fminf((float) p->tolerance, 1.0e30f) / ctx->tune_cluster_cell_div, &w.sb.grid));
    c.g = w.sb.grid.d;
    c.nf = n_finite;
    c.link_blocks = (unsigned) ((n_finite + kLinkBlock - 1) / kLinkBlock);
    const int rc = cl_back(ctx, w, c);
    if (rc != WM_OK && rc != WM_ERR_ARG) return rc;
    *n_out = c.kept;
    *n_clusters = c.m;
    if (stats) cl_stats_out(w.h_res.as<unsigned>(), n_finite, c.ms, stats);
    if (kernel_ms) *kernel_ms = c.ms;
    return rc;
}

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
    if (!ctx || !n_out || !n_clusters || (n > 0 && !pts) || n > 0x7FFFFFF0u || (cap > 0 && !indices_out) ||
        (cap_clusters > 0 && !offsets_out) || !cl_args_ok(p, stride, mem, out_mem))
        return WM_ERR_ARG;
    *n_out = 0;
    *n_clusters = 0;
    if (stats) *stats = wm_cluster_stats{};
    return cl_one(ctx, pts, n, stride, mem, p, labels_out, indices_out, cap, nullptr, 0, offsets_out, cap_clusters, out_mem,
                  n_clusters, n_out, stats, nullptr);
}

void wm_cluster_cond_default(wm_cluster_cond *c) {
    if (c) memset(c, 0, sizeof(*c));
}

int wm_cluster_extract_cond(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const void *attr, size_t attr_stride,
                            int attr_mem, const wm_cluster_params *p, const wm_cluster_cond *c, int32_t *labels_out,
                            int32_t *indices_out, size_t cap, uint32_t *offsets_out, size_t cap_clusters, int out_mem,
                            size_t *n_clusters, size_t *n_out, wm_cluster_stats *stats) {
    if (!ctx || !n_out || !n_clusters || (n > 0 && !pts) || n > 0x7FFFFFF0u || (cap > 0 && !indices_out) ||
        (cap_clusters > 0 && !offsets_out) || !cl_args_ok(p, stride, mem, out_mem))
        return WM_ERR_ARG;
    if (!c || c->flags < 0 || c->flags > (WM_CLUSTER_COND_NORMAL | WM_CLUSTER_COND_SCALAR) || c->reserved != 0 ||
        (c->flags != 0 && !attr && n > 0) || attr_stride < 16 || (attr_stride & 3) ||
        (attr_mem != WM_MEM_HOST && attr_mem != WM_MEM_DEVICE))
        return WM_ERR_ARG;
    if ((c->flags & WM_CLUSTER_COND_NORMAL) &&
        !(std::isfinite(c->max_normal_angle) && c->max_normal_angle >= 0.0 && c->max_normal_angle <= M_PI / 2))
        return WM_ERR_ARG;
    if ((c->flags & WM_CLUSTER_COND_SCALAR) && !(std::isfinite(c->max_scalar_diff) && c->max_scalar_diff >= 0.0))
        return WM_ERR_ARG;
    *n_out = 0;
    *n_clusters = 0;
    if (stats) *stats = wm_cluster_stats{};
    LinkCond lc{};
    lc.flags = c->flags;
    if (c->flags & WM_CLUSTER_COND_NORMAL) lc.cos_min = (float) cos(c->max_normal_angle);  // (the cosine in double)
    if (c->flags & WM_CLUSTER_COND_SCALAR) lc.max_diff = (float) c->max_scalar_diff;
    return cl_one(ctx, pts, n, stride, mem, p, labels_out, indices_out, cap, nullptr, 0, offsets_out, cap_clusters, out_mem,
                  n_clusters, n_out, stats, nullptr, &lc, attr, attr_stride, attr_mem);
}

int wm_cluster_extract_batch(wm_ctx *ctx, const wm_cluster_scan *scans, int n_scans, size_t stride, int mem,
                             const wm_cluster_params *p, int32_t *labels_out, int32_t *indices_out, size_t cap,
                             void *points_out, size_t out_stride, uint32_t *offsets_out, size_t cap_clusters, int out_mem,
                             size_t *cluster_first, size_t *n_out, wm_cluster_stats *stats, float *kernel_ms) {
    if (!ctx || n_scans < 0 || (n_scans > 0 && !scans) || !cluster_first || !n_out || (cap > 0 && !indices_out) ||
        (cap_clusters > 0 && !offsets_out) || (points_out && (out_stride < 12 || (out_stride & 3))) ||
        !cl_args_ok(p, stride, mem, out_mem) || (unsigned long long) n_scans > WM_CLUSTER_BATCH_MAX_SCANS)
        return WM_ERR_ARG;
    const unsigned S = (unsigned) n_scans;
    size_t total = 0, max_n = 0;
    for (unsigned k = 0; k < S; ++k) {
        if ((scans[k].n > 0 && !scans[k].pts) || scans[k].n > WM_CLUSTER_BATCH_MAX_POINTS) return WM_ERR_ARG;
        total += scans[k].n;
        if (total > WM_CLUSTER_BATCH_MAX_POINTS) return WM_ERR_ARG;
        max_n = std::max(max_n, scans[k].n);
    }
    // the sort key of a kept root: the scan, the size, the smallest index -- WM_CLUSTER_BATCH_KEY_BITS in all
    const unsigned field_bits = std::max(bits_of(max_n), 1u);
    if (S > 1 && bits_of(S - 1u) + 2u * field_bits > WM_CLUSTER_BATCH_KEY_BITS) return WM_ERR_ARG;
    *n_out = 0;
    for (unsigned k = 0; k <= S; ++k) cluster_first[k] = 0;
    if (stats)
        for (unsigned k = 0; k < S; ++k) stats[k] = wm_cluster_stats{};
    if (kernel_ms) *kernel_ms = 0.f;
    const bool host_out = out_mem == WM_MEM_HOST;
    if (S == 0 || total == 0) {  // (no device is touched)
        if (offsets_out && host_out) offsets_out[0] = 0;
        return WM_OK;
    }
    if (S == 1) {  // a batch of one is the single call: nothing to stage, nothing to amortise
        size_t m = 0;
        const int rc = cl_one(ctx, scans[0].pts, scans[0].n, stride, mem, p, labels_out, indices_out, cap, points_out,
                              out_stride, offsets_out, cap_clusters, out_mem, &m, n_out, stats, kernel_ms);
        cluster_first[1] = m;
        return rc;
    }
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->cluster) ctx->cluster = new ClusterWs();
    ClusterWs &w = *static_cast<ClusterWs *>(ctx->cluster);
    ClCall c;
    c.S = S;
    c.n = total;
    c.p = p;
    c.field_bits = field_bits;
    c.host_out = host_out;
    c.timed = true;  // (PairStage::submit records ev_a)
    c.labels_out = labels_out;
    c.indices_out = indices_out;
    c.cap = cap;
    c.points_out = points_out;
    c.out_stride = points_out ? out_stride : 0;
    c.offsets_out = offsets_out;
    c.cap_clusters = cap_clusters;

    // the front (wm_scan_batch.hpp): the table, the packed cloud, the lattices and the cell-sorted array
    ScanBatch b;
    WM_TRY(scan_batch_front(ctx, w.sb, scans, S, stride, mem, fminf((float) p->tolerance, 1.0e30f) / ctx->tune_cluster_cell_div,
                            (unsigned) kLinkBlock,
                            [&](unsigned k, ClScan &t) {
                                if (stats) stats[k].n_finite = t.nf;
                                return true;
                            },
                            &b));
    const ClScan *tab = b.tab;
    c.tab = b.d_tab;
    c.nf = b.nf_total;
    c.link_blocks = (unsigned) b.search_blocks;
    if (b.nf_total == 0) return cl_nothing_finite(ctx, w, c);
    c.g = GridDev{};
    c.g.pts = w.sb.grid.pts.as<float4>();

    const int rc = cl_back(ctx, w, c);
    if (rc != WM_OK && rc != WM_ERR_ARG) return rc;
    *n_out = c.kept;
    const unsigned *h = w.h_res.as<unsigned>();
    for (unsigned k = 0; k < S; ++k) {
        cluster_first[k + 1] = cluster_first[k] + h[4 * k + 1];
        if (stats) cl_stats_out(h + 4 * k, tab[k].nf, c.ms, &stats[k]);
    }
    if (kernel_ms) *kernel_ms = c.ms;
    return rc;
}

}  // extern "C"
