// wm_fpfh_radius.hip -- normals and FPFH descriptors over a RADIUS neighbourhood (pcl::NormalEstimation and
// pcl::FPFHEstimation with setRadiusSearch) as cloud-in / rows-out calls, wm_normals_radius and wm_fpfh_radius, shaped
// like wm_iss_keypoints: the call packs the cloud, builds a cell-sorted grid over it for this call alone, and works in
// a workspace of its own on the context.  The rule is in include/wavematch.h ("feature descriptors"); the checker is
// tests/fpfh_radius_reference.py.  Every sum that a neighbourhood forms is a sum of INTEGERS (int64, exact): the order
// in which a walk meets the neighbours -- the arrival order of the cell sort's atomics -- reaches no output.
//
//   front          pack_cloud, compute_bbox, build_call_grid: wm_outlier_filter's.  The cell is at least
//                  max(normal_radius, feature_radius) / fpfh_cell_div (default 2), ONE grid for every walk of the call.
//   k_nr_sums      one lane per finite point in grid order, one wave per workgroup; radius_walk<false>; the nine sums
//                  (three first moments, six second) in eighteen VGPRs -> sums_g (nine planes of int64, grid order), n_s.
//   k_nr_finish    one lane per finite point: normal_from_sums (wm_normal_rule.hpp, the text the host runs too) ->
//                  nrm_g (grid order, for the next walks' locality) and, through .w, the caller's arrays.  A kernel of
//                  its own: the double SVD needs the registers that the walk wants for its occupancy.
//   k_nrm_to_grid  a caller's normals into grid order instead.
//   k_spfh_radius  the first descriptor walk: per hit with 0 < d2 < r2 the pair features (wm_fpfh_pair.hpp) and one
//                  increment in each of the three histograms.  A count is at most 8191: eleven 13-bit fields in THREE
//                  64-bit words per histogram (4 + 4 + 3), the increment added to all three under a compare-select, so
//                  that no register array is indexed dynamically and nothing goes to LDS or scratch.  A point with more
//                  neighbours than that carries into the next field and nowhere else; the call then fails by its
//                  count.  Stores the counts as uint16 in grid order, a row of kSpfhRow (40) entries = five 16-byte
//                  words, and the wave's largest neighbour count (an integer atomic max: no order can show).
//   k_fpfh_weight_radius  the second walk: per hit W and the neighbour's row (five 16-byte loads, local in grid order),
//                  33 int64 accumulators in registers (count * W: 64-bit multiply-adds), the three totals, 33 floats to
//                  the caller's slot through .w.
//   the end        max_neighbors and n_valid come back in one copy, and the host waits once, behind it.
#include "wm_fpfh_pair.hpp"
#include "wm_iss_sums.hpp"
#include "wm_normal_rule.hpp"
#include "wm_radius_walk.hpp"

#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

constexpr int kFrBlock = 64;   // queries (threads) of a walk's workgroup: one wave, as k_iss_scatter
constexpr int kSpfhRow = 40;   // uint16 per point in the workspace: 33 counts and 7 zeros, five uint4
constexpr int kSpfhBits = 13;  // a count's field: 0 ... 8191
static_assert((1 << kSpfhBits) - 1 == WM_FPFH_RADIUS_MAX_NEIGHBORS, "a field holds the largest count");
static_assert(kFpfhDim == WM_FEATURE_DIM, "the descriptor's length in the header");
static_assert(kNormalScaleBits == 36, "the quantum the header states");

// ------------------------------------------------------------------ the nine sums of a normal
// sums_g: plane c (0 ... 2: x y z; 3 ... 8: xx xy xz yy yz zz) holds nf entries in grid order.  A hit is d2 < r2, the
// lane's own point among them.  |d| * scale1 and |product| * scale2 stay below 2^37 for a hit: inside iss_term's range.
__global__ void __launch_bounds__(kFrBlock)
    k_nr_sums(GridDev g, unsigned nf, float r2, float rf, double scale1, double scale2, long long *__restrict__ sums_g,
              int *__restrict__ ns_g) {
    __shared__ uint2 s_runs[kKnnRows * kFrBlock];
    const unsigned i = blockIdx.x * kFrBlock + threadIdx.x;
    if (i >= nf) return;
    const float4 q = g.pts[i];
    unsigned long long sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    unsigned hits = 0;
    radius_walk<false>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kFrBlock, [&](unsigned, const float4 &t) {
        if (g_d2(q.x, q.y, q.z, t) < r2) {
            const float fx = t.x - q.x, fy = t.y - q.y, fz = t.z - q.z;
            const double dx = (double) fx, dy = (double) fy, dz = (double) fz;
            sx += iss_term(dx, scale1);
            sy += iss_term(dy, scale1);
            sz += iss_term(dz, scale1);
            sxx += iss_term(dx * dx, scale2);
            sxy += iss_term(dx * dy, scale2);
            sxz += iss_term(dx * dz, scale2);
            syy += iss_term(dy * dy, scale2);
            syz += iss_term(dy * dz, scale2);
            szz += iss_term(dz * dz, scale2);
            ++hits;
        }
        return false;
    });
    const size_t p = nf;
    sums_g[i] = iss_unbias(sx, hits);
    sums_g[p + i] = iss_unbias(sy, hits);
    sums_g[2 * p + i] = iss_unbias(sz, hits);
    sums_g[3 * p + i] = iss_unbias(sxx, hits);
    sums_g[4 * p + i] = iss_unbias(sxy, hits);
    sums_g[5 * p + i] = iss_unbias(sxz, hits);
    sums_g[6 * p + i] = iss_unbias(syy, hits);
    sums_g[7 * p + i] = iss_unbias(syz, hits);
    sums_g[8 * p + i] = iss_unbias(szz, hits);
    ns_g[i] = (int) hits;
}

// normals_out / counts_out / sums_out: the caller's arrays (caller order), each may be null
__global__ void __launch_bounds__(kBlock)
    k_nr_finish(const float4 *__restrict__ gpts, unsigned nf, const long long *__restrict__ sums_g, const int *__restrict__ ns_g,
                int x, float4 *__restrict__ nrm_g, float4 *__restrict__ normals_out, int *__restrict__ counts_out,
                long long *__restrict__ sums_out) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    const size_t p = nf;
    long long s[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) s[c] = sums_g[c * p + i];
    const int n_s = ns_g[i];
    const float4 q = gpts[i];
    float r[4];
    normal_from_sums(s, n_s, x, q.x, q.y, q.z, r);
    const float4 res = make_float4(r[0], r[1], r[2], r[3]);
    nrm_g[i] = res;
    const unsigned w = __float_as_uint(q.w);
    if (normals_out) normals_out[w] = res;
    if (counts_out) counts_out[w] = n_s;
    if (sums_out) {
#pragma unroll
        for (int c = 0; c < 9; ++c) sums_out[(size_t) w * 9 + c] = s[c];
    }
}

__global__ void __launch_bounds__(kBlock)
    k_nrm_to_grid(const float4 *__restrict__ gpts, unsigned nf, const float4 *__restrict__ normals_in, float4 *__restrict__ nrm_g) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nf) return;
    nrm_g[i] = normals_in[__float_as_uint(gpts[i].w)];
}

__global__ void __launch_bounds__(kBlock) k_fr_fill(int *__restrict__ p, unsigned n, int v) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ the first descriptor walk
struct SpfhFields {
    unsigned long long w[3];  // bins 0 ... 3, 4 ... 7, 8 ... 10: 13 bits each
};
__device__ __forceinline__ void spfh_add(SpfhFields &h, int bin) {
    const unsigned long long inc = 1ull << (kSpfhBits * (bin & 3));
    const int word = bin >> 2;
    h.w[0] += word == 0 ? inc : 0ull;
    h.w[1] += word == 1 ? inc : 0ull;
    h.w[2] += word == 2 ? inc : 0ull;
}
__device__ __forceinline__ unsigned spfh_get(const SpfhFields &h, int bin) {  // (bin: a constant after unrolling)
    return (unsigned) (h.w[bin >> 2] >> (kSpfhBits * (bin & 3))) & (unsigned) WM_FPFH_RADIUS_MAX_NEIGHBORS;
}

// res[0]: the largest neighbour count.  spfh_g: kSpfhRow uint16 per point, grid order.  counts_out (n_f) and spfh_out
// (33 uint16 per point) are the caller's, in caller order, and may be null.
__global__ void __launch_bounds__(kFrBlock)
    k_spfh_radius(GridDev g, unsigned nf, float r2, float rf, const float4 *__restrict__ nrm_g, uint4 *__restrict__ spfh_g,
                  int *__restrict__ counts_out, unsigned short *__restrict__ spfh_out, unsigned *__restrict__ res) {
    __shared__ uint2 s_runs[kKnnRows * kFrBlock];
    const unsigned i = blockIdx.x * kFrBlock + threadIdx.x;
    const bool live = i < nf;
    unsigned hits = 0;
    if (live) {
        const float4 q = g.pts[i];
        const float4 np = nrm_g[i];
        const bool own = !(np.x == 0.f && np.y == 0.f && np.z == 0.f);
        SpfhFields h[3] = {{{0ull, 0ull, 0ull}}, {{0ull, 0ull, 0ull}}, {{0ull, 0ull, 0ull}}};
        radius_walk<false>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kFrBlock, [&](unsigned j, const float4 &t) {
            const float d2 = g_d2(q.x, q.y, q.z, t);
            if (d2 < r2 && d2 != 0.f) {
                ++hits;
                if (own) {
                    const float4 nq = nrm_g[j];
                    int bin[3];
                    if (fpfh_pair<true>(q.x, q.y, q.z, np, t, nq, d2, bin)) {  // (the IEEE roots of the rule)
#pragma unroll
                        for (int f = 0; f < 3; ++f) spfh_add(h[f], bin[f]);
                    }
                }
            }
            return false;
        });
        unsigned c[kSpfhRow / 2];
#pragma unroll
        for (int d = 0; d < kSpfhRow / 2; ++d) {
            const int b0 = 2 * d, b1 = 2 * d + 1;
            const unsigned lo = b0 < kFpfhDim ? spfh_get(h[b0 / kFpfhBins], b0 % kFpfhBins) : 0u;
            const unsigned hi = b1 < kFpfhDim ? spfh_get(h[b1 / kFpfhBins], b1 % kFpfhBins) : 0u;
            c[d] = lo | (hi << 16);
        }
        uint4 *row = spfh_g + (size_t) i * (kSpfhRow / 8);
#pragma unroll
        for (int v = 0; v < kSpfhRow / 8; ++v) row[v] = make_uint4(c[4 * v], c[4 * v + 1], c[4 * v + 2], c[4 * v + 3]);
        const unsigned w = __float_as_uint(q.w);
        if (counts_out) counts_out[w] = (int) hits;
        if (spfh_out) {
            unsigned short *o = spfh_out + (size_t) w * kFpfhDim;
#pragma unroll
            for (int b = 0; b < kFpfhDim; ++b) o[b] = (unsigned short) ((c[b >> 1] >> (16 * (b & 1))) & 0xFFFFu);
        }
    }
    unsigned m = hits;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned) __shfl_xor((int) m, off));
    if (threadIdx.x == 0 && m) atomicMax(res, m);
}

// ------------------------------------------------------------------ the second descriptor walk
// res[1]: the valid points.  out: 33 floats per point, caller order (zeroed for the points that are in no grid).
__global__ void __launch_bounds__(kFrBlock)
    k_fpfh_weight_radius(GridDev g, unsigned nf, float r2, float r2_floor, float rf, const float4 *__restrict__ nrm_g,
                         const uint4 *__restrict__ spfh_g, float *__restrict__ out, unsigned *__restrict__ res) {
    __shared__ uint2 s_runs[kKnnRows * kFrBlock];
    const unsigned i = blockIdx.x * kFrBlock + threadIdx.x;
    const bool live = i < nf;
    bool valid = false;
    if (live) {
        const float4 np = nrm_g[i];
        valid = !(np.x == 0.f && np.y == 0.f && np.z == 0.f);
    }
    const unsigned long long vote = __ballot(valid);
    if (threadIdx.x == 0 && vote) atomicAdd(res + 1, (unsigned) __popcll(vote));
    if (!live) return;
    const float4 q = g.pts[i];
    unsigned long long acc[kFpfhDim];
#pragma unroll
    for (int b = 0; b < kFpfhDim; ++b) acc[b] = 0ull;
    if (valid) {
        radius_walk<false>(g, q, rf * g.inv_h, s_runs, threadIdx.x, kFrBlock, [&](unsigned j, const float4 &t) {
            const float d2 = g_d2(q.x, q.y, q.z, t);
            if (d2 < r2 && d2 != 0.f) {
                const float ratio = __fdiv_rn(r2, fmaxf(d2, r2_floor));
                const unsigned long long W = (unsigned long long) (long long) rint((double) ratio * 1048576.0);
                const uint4 *row = spfh_g + (size_t) j * (kSpfhRow / 8);
                uint4 v[kSpfhRow / 8];
#pragma unroll
                for (int u = 0; u < kSpfhRow / 8; ++u) v[u] = row[u];
#pragma unroll
                for (int b = 0; b < kFpfhDim; ++b) {
                    const uint4 &s = v[b / 8];
                    const unsigned word = ((b / 2) & 3) == 0 ? s.x : (((b / 2) & 3) == 1 ? s.y : (((b / 2) & 3) == 2 ? s.z : s.w));
                    const unsigned cnt = (word >> (16 * (b & 1))) & 0xFFFFu;
                    acc[b] += (unsigned long long) cnt * W;
                }
            }
            return false;
        });
    }
    float *o = out + (size_t) __float_as_uint(q.w) * kFpfhDim;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
        unsigned long long total = 0ull;
#pragma unroll
        for (int b = 0; b < kFpfhBins; ++b) total += acc[f * kFpfhBins + b];
        const double dt = (double) (long long) total;
#pragma unroll
        for (int b = 0; b < kFpfhBins; ++b)
            o[f * kFpfhBins + b] = total ? (float) (((double) (long long) acc[f * kFpfhBins + b] * 100.0) / dt) : 0.f;
    }
}

}  // namespace

// The context's workspace of the two calls: its own buffers, shared with nothing else on the context.
struct FpfhRadiusWs {
    DevBuf pts;                   // the packed cloud
    GridLevel grid;               // its grid
    DevBuf sums, ns, nrm_g, spfh_g;  // grid order
    DevBuf nrm_in;                // a host caller's normals
    DevBuf nrm_c, counts_c, sums_c, fpfh_c, spfh_c;  // host outputs on their way
    DevBuf res;                   // max_neighbors, n_valid
    PinnedBuf h_res;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

void fpfh_radius_release(wm_ctx *ctx) {
    FpfhRadiusWs *w = static_cast<FpfhRadiusWs *>(ctx->fpfh_radius);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts,   &w->grid.pts, &w->grid.cell_start, &w->sums,   &w->ns,     &w->nrm_g,  &w->spfh_g, &w->nrm_in,
                      &w->nrm_c, &w->counts_c, &w->sums_c,          &w->fpfh_c, &w->spfh_c, &w->res};
    for (DevBuf *b : bufs) b->release();
    w->h_res.release();
    for (hipEvent_t e : w->ev)
        if (e) (void) hipEventDestroy(e);
    delete w;
    ctx->fpfh_radius = nullptr;
}

namespace {

unsigned fr_blocks(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

// (float) (r * r), the product in double, must be a normal float
bool fr_radius_ok(double r) {
    if (!std::isfinite(r) || !(r > 0)) return false;
    const float r2 = (float) (r * r);
    return std::isfinite(r2) && r2 >= FLT_MIN;
}

FpfhRadiusWs *fr_ws(wm_ctx *ctx) {
    if (ctx->fpfh_radius) return static_cast<FpfhRadiusWs *>(ctx->fpfh_radius);
    FpfhRadiusWs *w = new FpfhRadiusWs();
    for (hipEvent_t &e : w->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            for (hipEvent_t &d : w->ev)
                if (d) (void) hipEventDestroy(d);
            delete w;
            ctx->last_error = "hipEventCreate (radius descriptors)";
            return nullptr;
        }
    ctx->fpfh_radius = w;
    return w;
}

bool fr_cloud_args_ok(const wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, int out_mem) {
    return ctx && !(n > 0 && !pts) && stride >= 12 && !(stride & 3) && n <= WM_ISS_MAX_POINTS &&
           (mem == WM_MEM_HOST || mem == WM_MEM_DEVICE) && (out_mem == WM_MEM_HOST || out_mem == WM_MEM_DEVICE);
}

// the front: the packed cloud, its box and the call's grid (n_finite == 0: no grid)
int fr_front(wm_ctx *ctx, FpfhRadiusWs &w, const void *pts, size_t n, size_t stride, int mem, double max_radius, size_t *n_finite) {
    WM_HIP(ctx, w.pts.reserve(n * sizeof(float4)));
    float4 *cloud = w.pts.as<float4>();
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, cloud));
    Bbox bb;
    WM_TRY(compute_bbox(ctx, cloud, n, &bb, n_finite));
    if (*n_finite == 0) return WM_OK;
    const float floor_h = fminf((float) max_radius, 1.0e30f) / ctx->tune_fpfh_cell_div;
    return build_call_grid(ctx, cloud, n, *n_finite, bb, floor_h, &w.grid);
}

// the normals of the grid's points over `radius` -> w.nrm_g, and the caller's arrays where given (device pointers)
int fr_normals(wm_ctx *ctx, FpfhRadiusWs &w, size_t n_finite, double radius, float4 *normals_out, int *counts_out,
               long long *sums_out) {
    const float r2 = (float) (radius * radius);
    int x = 0;
    (void) frexpf(r2, &x);
    const double scale1 = ldexp(1.0, kNormalScaleBits - normal_half_exponent(x)), scale2 = ldexp(1.0, kNormalScaleBits - x);
    const unsigned nf = (unsigned) n_finite;
    WM_HIP(ctx, w.sums.reserve(n_finite * 9 * sizeof(long long)));
    WM_HIP(ctx, w.ns.reserve(n_finite * 4));
    WM_HIP(ctx, w.nrm_g.reserve(n_finite * sizeof(float4)));
    const GridDev g = w.grid.d;
    // (a point with float d2 < r2 lies within this of the query)
    hipLaunchKernelGGL(k_nr_sums, dim3((unsigned) ((n_finite + kFrBlock - 1) / kFrBlock)), dim3(kFrBlock), 0, ctx->stream, g, nf, r2,
                       sqrtf(r2) * 1.0001f, scale1, scale2, w.sums.as<long long>(), w.ns.as<int>());
    hipLaunchKernelGGL(k_nr_finish, dim3(fr_blocks(n_finite)), dim3(kBlock), 0, ctx->stream, g.pts, nf,
                       (const long long *) w.sums.as<long long>(), (const int *) w.ns.as<int>(), x, w.nrm_g.as<float4>(), normals_out,
                       counts_out, sums_out);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

}  // namespace

}  // namespace wm

using namespace wm;

extern "C" {

int wm_normal_from_sums(const int64_t sums[9], int n_s, int x, const float p[3], float out[4]) {
    if (!sums || !p || !out || n_s < 0 || x < -125 || x > 128) return WM_ERR_ARG;
    long long s[9];
    for (int c = 0; c < 9; ++c) s[c] = sums[c];
    normal_from_sums(s, n_s, x, p[0], p[1], p[2], out);
    return WM_OK;
}

int wm_normals_radius(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, double radius, float *normals_out,
                      int32_t *counts_out, int64_t *sums_out, int out_mem, wm_normals_radius_stats *stats) {
    if (!fr_cloud_args_ok(ctx, pts, n, stride, mem, out_mem) || !normals_out || !fr_radius_ok(radius)) return WM_ERR_ARG;
    if (stats) *stats = wm_normals_radius_stats{};
    if (n == 0) return WM_OK;  // (no device is touched)

    WM_HIP(ctx, hipSetDevice(ctx->device));
    FpfhRadiusWs *wp = fr_ws(ctx);
    if (!wp) return WM_ERR_HIP;
    FpfhRadiusWs &w = *wp;
    hipStream_t st = ctx->stream;
    const bool host_out = out_mem == WM_MEM_HOST;

    // the outputs' places: the caller's own in device memory, else the workspace's
    float4 *d_nrm = reinterpret_cast<float4 *>(normals_out);
    int *d_counts = reinterpret_cast<int *>(counts_out);
    long long *d_sums = reinterpret_cast<long long *>(sums_out);
    if (host_out) {
        WM_HIP(ctx, w.nrm_c.reserve(n * sizeof(float4)));
        d_nrm = w.nrm_c.as<float4>();
        if (counts_out) {
            WM_HIP(ctx, w.counts_c.reserve(n * 4));
            d_counts = w.counts_c.as<int>();
        }
        if (sums_out) {
            WM_HIP(ctx, w.sums_c.reserve(n * 9 * sizeof(long long)));
            d_sums = w.sums_c.as<long long>();
        }
    }
    WM_HIP(ctx, hipEventRecord(w.ev[0], st));
    size_t n_finite = 0;
    WM_TRY(fr_front(ctx, w, pts, n, stride, mem, radius, &n_finite));
    if (stats) stats->n_finite = n_finite;
    // what a point without a walk keeps: zeros, count -1
    if (n_finite != n) {
        WM_HIP(ctx, hipMemsetAsync(d_nrm, 0, n * sizeof(float4), st));
        if (d_sums) WM_HIP(ctx, hipMemsetAsync(d_sums, 0, n * 9 * sizeof(long long), st));
        if (d_counts) {
            hipLaunchKernelGGL(k_fr_fill, dim3(fr_blocks(n)), dim3(kBlock), 0, st, d_counts, (unsigned) n, -1);
            WM_HIP(ctx, hipGetLastError());
        }
    }
    if (n_finite > 0) WM_TRY(fr_normals(ctx, w, n_finite, radius, d_nrm, d_counts, d_sums));
    WM_HIP(ctx, hipEventRecord(w.ev[1], st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (stats) (void) hipEventElapsedTime(&stats->kernel_ms, w.ev[0], w.ev[1]);
    if (host_out) {
        WM_HIP(ctx, hipMemcpy(normals_out, d_nrm, n * sizeof(float4), hipMemcpyDeviceToHost));
        if (counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, n * 4, hipMemcpyDeviceToHost));
        if (sums_out) WM_HIP(ctx, hipMemcpy(sums_out, d_sums, n * 9 * sizeof(long long), hipMemcpyDeviceToHost));
    }
    return WM_OK;
}

int wm_fpfh_radius(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_fpfh_radius_params *p,
                   const void *normals_in, float *fpfh_out, uint16_t *spfh_out, int32_t *counts_out, int out_mem,
                   wm_fpfh_radius_stats *stats) {
    if (!fr_cloud_args_ok(ctx, pts, n, stride, mem, out_mem) || !p || !fpfh_out || !fr_radius_ok(p->feature_radius) ||
        (!normals_in && !fr_radius_ok(p->normal_radius)))
        return WM_ERR_ARG;
    if (stats) *stats = wm_fpfh_radius_stats{};
    if (n == 0) return WM_OK;  // (no device is touched)

    WM_HIP(ctx, hipSetDevice(ctx->device));
    FpfhRadiusWs *wp = fr_ws(ctx);
    if (!wp) return WM_ERR_HIP;
    FpfhRadiusWs &w = *wp;
    hipStream_t st = ctx->stream;
    const bool host_out = out_mem == WM_MEM_HOST;

    float *d_out = fpfh_out;
    unsigned short *d_spfh = spfh_out;
    int *d_counts = reinterpret_cast<int *>(counts_out);
    if (host_out) {
        WM_HIP(ctx, w.fpfh_c.reserve(n * kFpfhDim * sizeof(float)));
        d_out = w.fpfh_c.as<float>();
        if (spfh_out) {
            WM_HIP(ctx, w.spfh_c.reserve(n * kFpfhDim * sizeof(unsigned short)));
            d_spfh = w.spfh_c.as<unsigned short>();
        }
        if (counts_out) {
            WM_HIP(ctx, w.counts_c.reserve(n * 4));
            d_counts = w.counts_c.as<int>();
        }
    }
    WM_HIP(ctx, w.res.reserve(16));
    WM_HIP(ctx, w.h_res.reserve(16));
    unsigned *res = w.res.as<unsigned>();
    const float4 *d_nrm_in = static_cast<const float4 *>(normals_in);
    if (normals_in && mem == WM_MEM_HOST) {
        WM_HIP(ctx, w.nrm_in.reserve(n * sizeof(float4)));
        WM_HIP(ctx, hipMemcpyAsync(w.nrm_in.p, normals_in, n * sizeof(float4), hipMemcpyHostToDevice, st));
        d_nrm_in = w.nrm_in.as<float4>();
    }

    WM_HIP(ctx, hipEventRecord(w.ev[0], st));
    size_t n_finite = 0;
    const double max_radius = normals_in ? p->feature_radius : std::max(p->feature_radius, p->normal_radius);
    WM_TRY(fr_front(ctx, w, pts, n, stride, mem, max_radius, &n_finite));
    if (stats) stats->n_finite = n_finite;
    WM_HIP(ctx, hipMemsetAsync(res, 0, 16, st));
    if (n_finite != n) {
        WM_HIP(ctx, hipMemsetAsync(d_out, 0, n * kFpfhDim * sizeof(float), st));
        if (d_spfh) WM_HIP(ctx, hipMemsetAsync(d_spfh, 0, n * kFpfhDim * sizeof(unsigned short), st));
        if (d_counts) {
            hipLaunchKernelGGL(k_fr_fill, dim3(fr_blocks(n)), dim3(kBlock), 0, st, d_counts, (unsigned) n, -1);
            WM_HIP(ctx, hipGetLastError());
        }
    }
    WM_HIP(ctx, hipEventRecord(w.ev[1], st));
    if (n_finite > 0) {
        const unsigned nf = (unsigned) n_finite;
        const GridDev g = w.grid.d;
        if (normals_in) {
            WM_HIP(ctx, w.nrm_g.reserve(n_finite * sizeof(float4)));
            hipLaunchKernelGGL(k_nrm_to_grid, dim3(fr_blocks(n_finite)), dim3(kBlock), 0, st, g.pts, nf, d_nrm_in, w.nrm_g.as<float4>());
            WM_HIP(ctx, hipGetLastError());
        } else {
            WM_TRY(fr_normals(ctx, w, n_finite, p->normal_radius, nullptr, nullptr, nullptr));
        }
    }
    WM_HIP(ctx, hipEventRecord(w.ev[2], st));
    if (n_finite > 0) {
        const unsigned nf = (unsigned) n_finite;
        const GridDev g = w.grid.d;
        const float r2 = (float) (p->feature_radius * p->feature_radius);
        const float rf = sqrtf(r2) * 1.0001f;  // (a point with float d2 < r2 lies within this of the query)
        const unsigned walk_blocks = (unsigned) ((n_finite + kFrBlock - 1) / kFrBlock);
        WM_HIP(ctx, w.spfh_g.reserve(n_finite * kSpfhRow * sizeof(unsigned short)));
        hipLaunchKernelGGL(k_spfh_radius, dim3(walk_blocks), dim3(kFrBlock), 0, st, g, nf, r2, rf, (const float4 *) w.nrm_g.as<float4>(),
                           w.spfh_g.as<uint4>(), d_counts, d_spfh, res);
        WM_HIP(ctx, hipGetLastError());
        WM_HIP(ctx, hipEventRecord(w.ev[3], st));
        hipLaunchKernelGGL(k_fpfh_weight_radius, dim3(walk_blocks), dim3(kFrBlock), 0, st, g, nf, r2, r2 * (1.0f / 65536.0f), rf,
                           (const float4 *) w.nrm_g.as<float4>(), (const uint4 *) w.spfh_g.as<uint4>(), d_out, res);
        WM_HIP(ctx, hipGetLastError());
    } else {
        WM_HIP(ctx, hipEventRecord(w.ev[3], st));
    }
    WM_HIP(ctx, hipEventRecord(w.ev[4], st));
    WM_HIP(ctx, hipMemcpyAsync(w.h_res.p, res, 8, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));

    const unsigned *h = w.h_res.as<unsigned>();
    const size_t max_neighbors = h[0];
    if (stats) {
        stats->max_neighbors = max_neighbors;
        stats->n_valid = h[1];
        if (!normals_in) (void) hipEventElapsedTime(&stats->normals_ms, w.ev[1], w.ev[2]);
        (void) hipEventElapsedTime(&stats->spfh_ms, w.ev[2], w.ev[3]);
        (void) hipEventElapsedTime(&stats->weight_ms, w.ev[3], w.ev[4]);
        (void) hipEventElapsedTime(&stats->kernel_ms, w.ev[0], w.ev[4]);
    }
    if (max_neighbors > WM_FPFH_RADIUS_MAX_NEIGHBORS) return WM_ERR_ARG;  // (outside the call's range: the counts carried)
    if (host_out) {
        WM_HIP(ctx, hipMemcpy(fpfh_out, d_out, n * kFpfhDim * sizeof(float), hipMemcpyDeviceToHost));
        if (spfh_out) WM_HIP(ctx, hipMemcpy(spfh_out, d_spfh, n * kFpfhDim * sizeof(unsigned short), hipMemcpyDeviceToHost));
        if (counts_out) WM_HIP(ctx, hipMemcpy(counts_out, d_counts, n * 4, hipMemcpyDeviceToHost));
    }
    return WM_OK;
}

}  // extern "C"
