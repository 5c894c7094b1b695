// wm_iss.hip -- ISS keypoints on the device: pcl::ISSKeypoint3D (without its border estimation) as one cloud-in /
// indices-out call (wm_iss_keypoints), shaped like wm_outlier_filter: the call packs the cloud, builds a cell-sorted
// grid over it for this call alone, and works in a workspace of its own on the context.  The file also holds
// wm_gather_records, which picks the keypoints' descriptor rows for wm_feature_match without leaving the device.
//
// The rule is in include/wavematch.h ("keypoints"; written from PCL 1.8 keypoints/impl/iss_3d.hpp, PCL is not linked,
// the checker is tests/iss_reference.py).  In short: per finite point the scatter matrix of the differences to its
// neighbours within salient_radius, each of the six products an INTEGER of quantum 2^-36 of r2s, added in int64 -- a
// set of integers has one sum, so the order of the points inside a grid cell (the arrival order of the cell sort's
// atomics) reaches no output; its eigenvalues by jacobi3 (wm_iss_rule.hpp: one text for host and device); a salient
// point survives the non-maximum suppression iff no neighbour within non_max_radius has a larger third eigenvalue.
//
//   front        pack_cloud, compute_bbox, build_call_grid: wm_outlier_filter's.  The cell is at least
//                max(salient_radius, non_max_radius) / iss_cell_div (default 2), ONE grid for both walks.  Coarser
//                cells change no output: the walks are exact whatever the lattice.
//   k_iss_scatter  one lane per finite point in grid order, one wave per workgroup; radius_walk<false>; the six sums in
//                twelve VGPRs -> sums_g (six planes of int64, grid order) and n_s.
//   k_iss_third  one lane per finite point: iss_third -> third_g (grid order, for the next walk's locality) and, through
//                .w, third_out and counts_out when the caller wants them.  A kernel of its own: the double Jacobi step
//                needs the registers that the walk wants for its occupancy.
//   k_iss_nms    one lane per finite point in grid order; a lane with third == 0 does not walk, the others run
//                radius_walk<true> and leave it at the first neighbour with a larger third.  Writes the point's label
//                and its keep flag through .w (caller order), and counts the salient points (an integer atomic per
//                wave: no order can show).
//   compaction   ONE exclusive scan of the keep flags over caller positions and k_iss_emit: the keypoints' indices
//                ascending; the number of keypoints goes behind the salient count.
//   the end      both counters come back in one copy, and the host waits once, behind it.
#include "wm_iss_rule.hpp"
#include "wm_iss_sums.hpp"
#include "wm_radius_walk.hpp"

#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

constexpr int kIssBlock = 64;  // queries (threads) of a walk's workgroup: one wave, as k_outlier_radius

// ------------------------------------------------------------------ the scatter sums
// sums_g: plane c (0 ... 5: xx xy xz yy yz zz) holds nf entries in grid order.  A hit is d2 < r2s, the lane's own
// point among them (d2 = 0 < r2s).  |product| * scale < 2^37 for a hit: the terms are far inside iss_term's range.
__global__ void __launch_bounds__(kIssBlock)
    k_iss_scatter(GridDev g, unsigned nf, float r2, float rf, double scale, long long *__restrict__ sums_g, int *__restrict__ ns_g) {
    __shared__ uint2 s_runs[kKnnRows * kIssBlock];
    const unsigned i = blockIdx.x * kIssBlock + threadIdx.x;
    if (i >= nf) return;
    const float4 q = g.pts[i];
    unsigned long long sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    unsigned hits = 0;
    radius_walk<false>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kIssBlock, [&](unsigned, const float4 &t) {
        if (g_d2(q.x, q.y, q.z, t) < r2) {
            const float fx = t.x - q.x, fy = t.y - q.y, fz = t.z - q.z;
            const double dx = (double) fx, dy = (double) fy, dz = (double) fz;
            sxx += iss_term(dx * dx, scale);
            sxy += iss_term(dx * dy, scale);
            sxz += iss_term(dx * dz, scale);
            syy += iss_term(dy * dy, scale);
            syz += iss_term(dy * dz, scale);
            szz += iss_term(dz * dz, scale);
            ++hits;
        }
        return false;
    });
    const size_t p = nf;
    sums_g[i] = iss_unbias(sxx, hits);
    sums_g[p + i] = iss_unbias(sxy, hits);
    sums_g[2 * p + i] = iss_unbias(sxz, hits);
    sums_g[3 * p + i] = iss_unbias(syy, hits);
    sums_g[4 * p + i] = iss_unbias(syz, hits);
    sums_g[5 * p + i] = iss_unbias(szz, hits);
    ns_g[i] = (int) hits;
}

// ------------------------------------------------------------------ the saliency step
__global__ void __launch_bounds__(kBlock)
    k_iss_third(const float4 *__restrict__ gpts, unsigned nf, const long long *__restrict__ sums_g, const int *__restrict__ ns_g,
                int min_neighbors, int x, double gamma_21, double gamma_32, double *__restrict__ third_g,
                double *__restrict__ third_out, int *__restrict__ counts_out) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const size_t p = nf;
    const long long s[6] = {sums_g[i], sums_g[p + i], sums_g[2 * p + i], sums_g[3 * p + i], sums_g[4 * p + i], sums_g[5 * p + i]};
    const int n_s = ns_g[i];
    const double third = iss_third(s, n_s, min_neighbors, x, gamma_21, gamma_32);
    third_g[i] = third;
    if (third_out || counts_out) {
        const unsigned w = __float_as_uint(gpts[i].w);
        if (third_out) third_out[w] = third;
        if (counts_out) counts_out[w] = n_s;
    }
}

// ------------------------------------------------------------------ the non-maximum suppression
// labels and keep were cleared (NONE, 0): a non-finite point is in no grid and keeps both.  res[0]: the salient points.
__global__ void __launch_bounds__(kIssBlock)
    k_iss_nms(GridDev g, unsigned nf, float r2, float rf, unsigned min_neighbors, const double *__restrict__ third_g,
              uint8_t *__restrict__ labels, unsigned *__restrict__ keep, unsigned *__restrict__ res) {
    __shared__ uint2 s_runs[kKnnRows * kIssBlock];
    const unsigned i = blockIdx.x * kIssBlock + threadIdx.x;
    const bool live = i < nf;
    const double mine = live ? third_g[i] : 0.0;
    const bool salient = mine > 0.0;
    const unsigned long long m = __ballot(salient);
    if (threadIdx.x == 0 && m) atomicAdd(res, (unsigned) __popcll(m));
    if (!live) return;
    const float4 q = g.pts[i];
    const unsigned w = __float_as_uint(q.w);
    bool key = false;
    if (salient) {
        unsigned hits = 0;
        bool beaten = false;
        // (third_g[j] waits for the distance test.  Asking for candidate j + 1's value while j is tested, 8 B for every
        // candidate beside the walk's own point load, was measured 3 - 12 % slower: DESIGN.md 4.16)
        radius_walk<true>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kIssBlock, [&](unsigned j, const float4 &t) {
            if (g_d2(q.x, q.y, q.z, t) < r2) {
                ++hits;
                beaten = third_g[j] > mine;
            }
            return beaten;
        });
        key = !beaten && hits >= min_neighbors;
    }
    labels[w] = (uint8_t) (key ? WM_ISS_KEYPOINT : (salient ? WM_ISS_SALIENT : WM_ISS_PLAIN));
    if (key) keep[w] = 1u;
}

// pos = the exclusive scan of keep over caller positions (n + 1 entries): the keypoints ascending; res[1] = their number
__global__ void __launch_bounds__(kBlock)
    k_iss_emit(unsigned n, const unsigned *__restrict__ keep, const unsigned *__restrict__ pos, int *__restrict__ out, size_t cap,
               unsigned *__restrict__ res) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) res[1] = pos[n];
    if (i >= n || !keep[i]) return;
    const unsigned j = pos[i];
    if (j < cap) out[j] = (int) i;
}

__global__ void __launch_bounds__(kBlock) k_iss_fill(int *__restrict__ p, unsigned n, int v) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ wm_gather_records
// dst record j = src record idx[j], in words of four bytes; a thread takes words t, t + T, ...  An index outside
// [0, n) reads nothing, writes nothing and is counted (once, by the thread of its first word).
__global__ void __launch_bounds__(kBlock)
    k_gather_records(const uint32_t *__restrict__ src, unsigned n, unsigned words, const int *__restrict__ idx, size_t total,
                     uint32_t *__restrict__ dst, unsigned *__restrict__ bad) {
    const size_t step = (size_t) gridDim.x * kBlock;
    for (size_t t = (size_t) blockIdx.x * kBlock + threadIdx.x; t < total; t += step) {
        const size_t j = t / words;
        const unsigned k = (unsigned) (t - j * words);
        const int s = idx[j];
        if (s < 0 || (unsigned) s >= n) {
            if (k == 0) atomicAdd(bad, 1u);
            continue;
        }
        dst[t] = src[(size_t) s * words + k];
    }
}

}  // namespace

// The context's workspace of the keypoint detector: its own buffers, shared with nothing else on the context.
struct IssWs {
    DevBuf pts;                 // the packed cloud
    GridLevel grid;             // its grid
    DevBuf sums, ns, third_g;   // grid order
    DevBuf labels, keep, pos;   // caller order
    DevBuf third_c, counts_c, out;  // host outputs on their way
    DevBuf res;                 // n_salient, n_keypoints; wm_gather_records' bad indices
    PinnedBuf h_res;
};

void iss_release(wm_ctx *ctx) {
    IssWs *w = static_cast<IssWs *>(ctx->iss);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts, &w->grid.pts, &w->grid.cell_start, &w->sums, &w->ns, &w->third_g, &w->labels, &w->keep,
                      &w->pos, &w->third_c, &w->counts_c, &w->out, &w->res};
    for (DevBuf *b : bufs) b->release();
    w->h_res.release();
    delete w;
    ctx->iss = nullptr;
}

namespace {

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

// (float) (r * r), the product in double, must be a normal float
bool iss_radius_ok(double r) {
    if (!std::isfinite(r) || !(r > 0)) return false;
    const float r2 = (float) (r * r);
    return std::isfinite(r2) && r2 >= FLT_MIN;
}

bool iss_params_ok(const wm_iss_params *p) {
    return iss_radius_ok(p->salient_radius) && iss_radius_ok(p->non_max_radius) && std::isfinite(p->gamma_21) &&
           p->gamma_21 >= 0 && std::isfinite(p->gamma_32) && p->gamma_32 >= 0 && p->min_neighbors >= 0;
}

IssWs &iss_ws(wm_ctx *ctx) {
    if (!ctx->iss) ctx->iss = new IssWs();
    return *static_cast<IssWs *>(ctx->iss);
}

}  // namespace

}  // namespace wm

using namespace wm;

extern "C" {

void wm_iss_default_params(wm_iss_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->salient_radius = 0.0;  // iss_3d.h: salient_radius_ (0.0001) and non_max_radius_ (0.0) are no usable defaults
    p->non_max_radius = 0.0;
    p->gamma_21 = 0.975;
    p->gamma_32 = 0.975;
    p->min_neighbors = 5;
}

int wm_iss_third(const int64_t sums[6], int n_s, int x, const wm_iss_params *p, double *third_out) {
    if (!sums || !p || !third_out || !std::isfinite(p->gamma_21) || p->gamma_21 < 0 || !std::isfinite(p->gamma_32) ||
        p->gamma_32 < 0 || p->min_neighbors < 0 || x < -125 || x > 128)
        return WM_ERR_ARG;
    const long long s[6] = {sums[0], sums[1], sums[2], sums[3], sums[4], sums[5]};
    *third_out = iss_third(s, n_s, p->min_neighbors, x, p->gamma_21, p->gamma_32);
    return WM_OK;
}

int wm_iss_keypoints(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_iss_params *p,
                     int32_t *indices_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out, double *third_out,
                     int32_t *counts_out, wm_iss_stats *stats) {
    if (!ctx || !p || !n_out || (n > 0 && !pts) || stride < 12 || (stride & 3) || n > WM_ISS_MAX_POINTS ||
        (cap > 0 && !indices_out) || (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) ||
        (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE) || !iss_params_ok(p))
        return WM_ERR_ARG;
    *n_out = 0;
    if (stats) *stats = wm_iss_stats{};
    if (n == 0) return WM_OK;  // (no device is touched)

    WM_HIP(ctx, hipSetDevice(ctx->device));
    IssWs &w = iss_ws(ctx);
    hipStream_t st = ctx->stream;
    const bool host_out = out_mem == WM_MEM_HOST;
    const unsigned blocks = blocks_of(n);

    // the outputs' places: the caller's own in device memory, else the workspace's
    WM_HIP(ctx, w.pts.reserve(n * sizeof(float4)));
    WM_HIP(ctx, w.keep.reserve(n * 4));
    WM_HIP(ctx, w.pos.reserve((n + 1) * 4));
    WM_HIP(ctx, w.res.reserve(16));
    WM_HIP(ctx, w.h_res.reserve(16));
    uint8_t *d_labels = labels_out;
    if (host_out || !labels_out) {
        WM_HIP(ctx, w.labels.reserve(n));
        d_labels = w.labels.as<uint8_t>();
    }
    double *d_third = third_out;
    if (third_out && host_out) {
        WM_HIP(ctx, w.third_c.reserve(n * 8));
        d_third = w.third_c.as<double>();
    }
    int *d_counts = counts_out;
    if (counts_out && host_out) {
        WM_HIP(ctx, w.counts_c.reserve(n * 4));
        d_counts = w.counts_c.as<int>();
    }
    const size_t d_cap = std::min(cap, n);
    int *d_out = reinterpret_cast<int *>(indices_out);
    if (host_out) {
        WM_HIP(ctx, w.out.reserve(d_cap * 4));
        d_out = w.out.as<int>();
    }
    unsigned *res = w.res.as<unsigned>();

    if (stats) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    float4 *cloud = w.pts.as<float4>();
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, cloud));
    Bbox bb;
    size_t n_finite = 0;
    WM_TRY(compute_bbox(ctx, cloud, n, &bb, &n_finite));
    if (stats) stats->n_finite = n_finite;

    // what a point without a walk keeps: label NONE, third 0, count -1, not kept
    WM_HIP(ctx, hipMemsetAsync(d_labels, 0, n, st));
    WM_HIP(ctx, hipMemsetAsync(w.keep.p, 0, n * 4, st));
    WM_HIP(ctx, hipMemsetAsync(res, 0, 16, st));
    if (d_third) WM_HIP(ctx, hipMemsetAsync(d_third, 0, n * 8, st));
    if (d_counts) {
        hipLaunchKernelGGL(k_iss_fill, dim3(blocks), dim3(kBlock), 0, st, d_counts, (unsigned) n, -1);
        WM_HIP(ctx, hipGetLastError());
    }

    if (n_finite > 0) {
        const float r2s = (float) (p->salient_radius * p->salient_radius);
        const float r2n = (float) (p->non_max_radius * p->non_max_radius);
        int x = 0;
        (void) frexpf(r2s, &x);
        const double scale = ldexp(1.0, kIssScaleBits - x);
        const float floor_h = fminf((float) std::max(p->salient_radius, p->non_max_radius), 1.0e30f) / ctx->tune_iss_cell_div;
        WM_TRY(build_call_grid(ctx, cloud, n, n_finite, bb, floor_h, &w.grid));
        const GridDev g = w.grid.d;
        const unsigned nf = (unsigned) n_finite;
        WM_HIP(ctx, w.sums.reserve(n_finite * 6 * sizeof(long long)));
        WM_HIP(ctx, w.ns.reserve(n_finite * 4));
        WM_HIP(ctx, w.third_g.reserve(n_finite * 8));
        const unsigned walk_blocks = (unsigned) ((n_finite + kIssBlock - 1) / kIssBlock);
        // (a point with float d2 < r2 lies within this of the query)
        hipLaunchKernelGGL(k_iss_scatter, dim3(walk_blocks), dim3(kIssBlock), 0, st, g, nf, r2s, sqrtf(r2s) * 1.0001f, scale,
                           w.sums.as<long long>(), w.ns.as<int>());
        hipLaunchKernelGGL(k_iss_third, dim3(blocks_of(n_finite)), dim3(kBlock), 0, st, g.pts, nf,
                           (const long long *) w.sums.as<long long>(), (const int *) w.ns.as<int>(), p->min_neighbors, x,
                           p->gamma_21, p->gamma_32, w.third_g.as<double>(), d_third, d_counts);
        hipLaunchKernelGGL(k_iss_nms, dim3(walk_blocks), dim3(kIssBlock), 0, st, g, nf, r2n, sqrtf(r2n) * 1.0001f,
                           (unsigned) p->min_neighbors, (const double *) w.third_g.as<double>(), d_labels, w.keep.as<unsigned>(),
                           res);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(exclusive_scan(ctx, w.keep.as<unsigned>(), n, w.pos.as<unsigned>()));
        hipLaunchKernelGGL(k_iss_emit, dim3(blocks), dim3(kBlock), 0, st, (unsigned) n, (const unsigned *) w.keep.as<unsigned>(),
                           (const unsigned *) w.pos.as<unsigned>(), d_out, d_cap, res);
        WM_HIP(ctx, hipGetLastError());
    }
    if (stats) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipMemcpyAsync(w.h_res.p, res, 8, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));

    const unsigned *h = w.h_res.as<unsigned>();
    const size_t kept = h[1];
    *n_out = kept;
    if (stats) {
        stats->n_salient = h[0];
        stats->n_keypoints = kept;
        (void) hipEventElapsedTime(&stats->kernel_ms, ctx->ev_a, ctx->ev_b);
    }
    if (host_out) {
        const size_t m = std::min(kept, cap);
        if (m) WM_HIP(ctx, hipMemcpy(indices_out, d_out, m * 4, hipMemcpyDeviceToHost));
        if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, n, hipMemcpyDeviceToHost));
        if (third_out) WM_HIP(ctx, hipMemcpy(third_out, d_third, n * 8, hipMemcpyDeviceToHost));
        if (counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, n * 4, hipMemcpyDeviceToHost));
    }
    return kept > cap ? WM_ERR_ARG : WM_OK;
}

int wm_gather_records(wm_ctx *ctx, const void *src, size_t n, size_t stride, const int32_t *idx, size_t m, void *dst, int mem) {
    if (!ctx || stride == 0 || (stride & 3) || stride > WM_GATHER_MAX_STRIDE || n > 0x7FFFFFF0u || m > 0x7FFFFFF0u || (n > 0 && !src) ||
        (m > 0 && (!idx || !dst)) || (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE))
        return WM_ERR_ARG;
    if (m == 0) return WM_OK;  // (no device is touched)
    if (mem == WM_MEM_HOST) {
        for (size_t j = 0; j < m; ++j)
            if (idx[j] < 0 || (size_t) idx[j] >= n) return WM_ERR_ARG;
        for (size_t j = 0; j < m; ++j)
            memcpy(static_cast<unsigned char *>(dst) + j * stride, static_cast<const unsigned char *>(src) + (size_t) idx[j] * stride,
                   stride);
        return WM_OK;
    }
    WM_HIP(ctx, hipSetDevice(ctx->device));
    IssWs &w = iss_ws(ctx);
    hipStream_t st = ctx->stream;
    WM_HIP(ctx, w.res.reserve(16));
    WM_HIP(ctx, w.h_res.reserve(16));
    unsigned *bad = w.res.as<unsigned>() + 2;
    WM_HIP(ctx, hipMemsetAsync(bad, 0, 4, st));
    const unsigned words = (unsigned) (stride / 4);
    const size_t total = m * words;
    const unsigned blocks = (unsigned) std::min<size_t>((total + kBlock - 1) / kBlock, 1u << 20);
    hipLaunchKernelGGL(k_gather_records, dim3(blocks), dim3(kBlock), 0, st, static_cast<const uint32_t *>(src), (unsigned) n, words,
                       reinterpret_cast<const int *>(idx), total, static_cast<uint32_t *>(dst), bad);
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipMemcpyAsync(w.h_res.as<unsigned>() + 2, bad, 4, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    return w.h_res.as<unsigned>()[2] ? WM_ERR_ARG : WM_OK;
}

}  // extern "C"
