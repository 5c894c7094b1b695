// wm_sac.hip -- plane segmentation on the device: pcl::SACSegmentation with a plane model and SAC_RANSAC as one cloud-in /
// plane-out call (wm_sac_segment), shaped like wm_cluster_extract: the call packs the cloud and works in a workspace of
// its own on the context.  No grid, no neighbour search: the hot loop is hypotheses x points plane tests.
//
// The rule is stated in include/wavematch.h (written from PCL 1.8 ransac.hpp, sac_model_plane.hpp and
// sac_segmentation.hpp; PCL is not linked, the checker is tests/sac_reference.py).  The hypothesis stream is a function
// of (seed, j, n), so the device evaluates it in ROUNDS of up to `sac_round` entries and the host walks each round's
// (flag, count) pairs in stream order with PCL's loop; entries behind the stopping point are discarded.  A round never
// holds more entries than the loop can still count as iterations (max_iterations + 1 - it): only skipped entries make
// another round necessary.  How the stream is cut into rounds changes no output.
//
// Launches of a call: pack, then per round
//   k_sac_hypotheses   one lane per stream entry: indices -> three point loads -> plane -> validity; a float4 and a flag
//   k_sac_count        the hot kernel: a lane keeps kSacPts points in registers and loops over the round's planes, read
//                      through a wave-uniform index (scalar loads); per plane a ballot and a popcount per point slot,
//                      accumulated per workgroup in LDS; one integer atomicAdd per plane and workgroup at its end.
//                      Integer counts: order-independent.  The points are read once per round.
//   one fetch of the round (planes, flags, counts)
// and behind the loop k_sac_sums (the refit's nine sums of the model's inliers as exact integer limbs, wm_bins.hpp's
// splitting with a bins array of this call's own) + one fetch of the limbs, the 3 x 3 eigenproblem on the host, then
// k_sac_select (flags and labels) -> exclusive_scan -> k_sac_compact and one fetch of the count.
#include <float.h>
#include <string.h>

#include "wm_bins.hpp"

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

constexpr int kSacMaxRound = 1024;            // the option's upper end: s_cnt of k_sac_count
constexpr int kSacPts = 4;                    // points a lane of k_sac_count keeps in registers
constexpr int kSacTile = kBlock * kSacPts;    // points of a workgroup's tile
constexpr unsigned kSacMaxBlocks = 2048;      // workgroups of k_sac_count at the most (8 per CU): each walks tiles
// the refit's bins: kSacBins bins x kBinLimbs limb rows x kSacStride words; components 0 ... 8 in use ([0..2] sum dx dy
// dz, [3..8] sum dxdx dxdy dxdz dydy dydz dzdz), word kSacPoison of limb row 0 counts sums the limbs cannot hold.
// A limb of one addend is below 2^40 and a bin's word holds 2^63: 2^23 points per bin, 2^31 points over 256 bins.
constexpr int kSacBins = 256;
constexpr int kSacStride = 16;
constexpr int kSacComps = 9;
constexpr int kSacPoison = kSacStride - 1;
constexpr size_t kSacBinWords = (size_t) kSacBins * kBinLimbs * kSacStride;

enum : unsigned { kSacSkipped = 0u, kSacValid = 1u, kSacAxisInvalid = 2u };

// ------------------------------------------------------------------ the hypothesis stream (host and device)
WM_HD unsigned long long sac_sm64(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
WM_HD unsigned sac_r(unsigned long long seed, unsigned long long j, unsigned a, unsigned m) {
    const unsigned long long h = sac_sm64(seed + 0x9E3779B97F4A7C15ull * (3ull * j + a + 1ull));
    return (unsigned) (((h >> 32) * (unsigned long long) m) >> 32);
}
// (n >= 3)
WM_HD void sac_sample(unsigned long long seed, unsigned long long j, unsigned n, unsigned (&i)[3]) {
    i[0] = sac_r(seed, j, 0u, n);
    unsigned t = sac_r(seed, j, 1u, n - 1u);
    i[1] = t + (t >= i[0] ? 1u : 0u);
    const unsigned lo = i[0] < i[1] ? i[0] : i[1], hi = i[0] < i[1] ? i[1] : i[0];
    t = sac_r(seed, j, 2u, n - 2u);
    t += t >= lo ? 1u : 0u;
    t += t >= hi ? 1u : 0u;
    i[2] = t;
}

// dist = |((a x + b y) + c z) + d|, every operation rounded
__device__ __forceinline__ float sac_dist(const float4 &pl, float x, float y, float z) {
    return fabsf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(pl.x, x), __fmul_rn(pl.y, y)), __fmul_rn(pl.z, z)), pl.w));
}

struct SacAxis {
    int model;
    float x, y, z, cos_eps, sin_eps;
};

// One lane per entry j0 + e of the round.  counts[e] = 0 for the count kernel behind it.
__global__ void __launch_bounds__(kBlock)
    k_sac_hypotheses(const float4 *__restrict__ pts, unsigned n, unsigned long long seed, unsigned long long j0, unsigned R,
                     SacAxis ax, float4 *__restrict__ planes, unsigned *__restrict__ flags, unsigned *__restrict__ counts) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= R) return;
    unsigned i[3];
    sac_sample(seed, j0 + e, n, i);  // (each index < n by construction)
    const float4 p0 = pts[i[0]], p1 = pts[i[1]], p2 = pts[i[2]];
    const float ux = __fsub_rn(p1.x, p0.x), uy = __fsub_rn(p1.y, p0.y), uz = __fsub_rn(p1.z, p0.z);
    const float vx = __fsub_rn(p2.x, p0.x), vy = __fsub_rn(p2.y, p0.y), vz = __fsub_rn(p2.z, p0.z);
    const float cx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
    const float cy = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
    const float cz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz));
    unsigned flag = kSacSkipped;
    float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
    if (isfinite(s) && s > 0.f) {
        const float l = sqrtf(s);  // (correctly rounded, as wm_ground.hip's: HIP's __fsqrt_rn is the native approximation)
        pl.x = __fdiv_rn(cx, l);
        pl.y = __fdiv_rn(cy, l);
        pl.z = __fdiv_rn(cz, l);
        pl.w = -__fadd_rn(__fadd_rn(__fmul_rn(pl.x, p0.x), __fmul_rn(pl.y, p0.y)), __fmul_rn(pl.z, p0.z));
        flag = kSacValid;
        if (ax.model != WM_SAC_PLANE) {
            const float dot = fabsf(__fadd_rn(__fadd_rn(__fmul_rn(pl.x, ax.x), __fmul_rn(pl.y, ax.y)), __fmul_rn(pl.z, ax.z)));
            const bool ok = ax.model == WM_SAC_PERPENDICULAR_PLANE ? dot >= ax.cos_eps : dot < ax.sin_eps;
            if (!ok) flag = kSacAxisInvalid;
        }
    }
    planes[e] = pl;
    flags[e] = flag;
    counts[e] = 0u;
}

// The hot kernel.  A workgroup walks tiles of kSacTile points; of a tile a lane holds kSacPts points (slot u: point
// tile * kSacTile + u * kBlock + thread, coalesced) and tests them against every valid plane of the round.  planes and
// flags are read at a wave-uniform index.  A point behind the cloud's end and a non-finite point (NaN since the pack)
// fail dist < thr.  finite_out != nullptr (the first round): the cloud's finite points are counted on the way.
__global__ void __launch_bounds__(kBlock)
    k_sac_count(const float4 *__restrict__ pts, unsigned n, const float4 *__restrict__ planes,
                const unsigned *__restrict__ flags, unsigned R, float thr, unsigned *__restrict__ counts,
                unsigned *__restrict__ finite_out) {
    __shared__ unsigned s_cnt[kSacMaxRound];
    for (unsigned j = threadIdx.x; j < R; j += kBlock) s_cnt[j] = 0u;
    __syncthreads();
    const bool lane0 = (threadIdx.x & 63u) == 0u;
    const float nanv = __builtin_nanf("");
    unsigned nfin = 0u;
    for (size_t t0 = (size_t) blockIdx.x * kSacTile; t0 < n; t0 += (size_t) gridDim.x * kSacTile) {
        float x[kSacPts], y[kSacPts], z[kSacPts];
#pragma unroll
        for (int u = 0; u < kSacPts; ++u) {
            const size_t i = t0 + (size_t) u * kBlock + threadIdx.x;
            x[u] = y[u] = z[u] = nanv;
            if (i < n) {
                const float4 p = pts[i];
                x[u] = p.x;
                y[u] = p.y;
                z[u] = p.z;
            }
            if (finite_out) nfin += (unsigned) __popcll(__ballot(x[u] == x[u]));
        }
        float4 pl_next = planes[0];  // (R >= 1) the next plane's scalar loads run under this plane's tests
        unsigned flag_next = flags[0];
        for (unsigned j = 0; j < R; ++j) {
            const float4 pl = pl_next;
            const unsigned flag = flag_next;
            const unsigned jn = j + 1u < R ? j + 1u : j;
            pl_next = planes[jn];
            flag_next = flags[jn];
            if (flag != kSacValid) continue;  // (the same for every lane)
            unsigned c = 0u;
#pragma unroll
            for (int u = 0; u < kSacPts; ++u) c += (unsigned) __popcll(__ballot(sac_dist(pl, x[u], y[u], z[u]) < thr));
            if (lane0 && c) atomicAdd(&s_cnt[j], c);
        }
    }
    __syncthreads();
    for (unsigned j = threadIdx.x; j < R; j += kBlock)
        if (s_cnt[j]) atomicAdd(&counts[j], s_cnt[j]);
    if (finite_out && lane0 && nfin) atomicAdd(finite_out, nfin);
}

// The refit's sums over the MODEL's inliers, relative to p0 = pts[i0] (the winning sample's first point, finite since
// its entry was valid).  A point's nine terms are doubles formed from exact differences, each split into limbs
// (bins_split: a function of the term alone); the limbs are integers, so the wave's shuffles and the bins' atomics add
// them exactly in any order.  tail: the words behind the bins, where p0 goes for the host.
__global__ void __launch_bounds__(kBlock)
    k_sac_sums(const float4 *__restrict__ pts, unsigned n, float4 pl, float thr, unsigned i0, long long *__restrict__ bins,
               float4 *__restrict__ tail) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const float4 p0 = pts[i0];
    if (i == 0u) *tail = p0;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool in = false;
    if (i < n) {
        p = pts[i];
        in = sac_dist(pl, p.x, p.y, p.z) < thr;
    }
    if (__ballot(in) == 0ull) return;  // (the whole wave)
    const double dx = in ? (double) p.x - (double) p0.x : 0.0, dy = in ? (double) p.y - (double) p0.y : 0.0,
                 dz = in ? (double) p.z - (double) p0.z : 0.0;
    const double term[kSacComps] = {dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
    const unsigned wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    long long *b = bins + (size_t) (wave % kSacBins) * (kBinLimbs * kSacStride);
    bool poison = false;
#pragma unroll
    for (int c = 0; c < kSacComps; ++c) {
        long long l[kBinLimbs] = {0ll, 0ll, 0ll};
        if (fabs(term[c]) < 4611686018427387904.0) bins_split(term[c], l);  // (2^62)
        else poison = true;
#pragma unroll
        for (int k = 0; k < kBinLimbs; ++k) {
            long long v = l[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if ((threadIdx.x & 63u) == 0u && v != 0ll)
                (void) __hip_atomic_fetch_add(b + k * kSacStride + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (__ballot(poison) != 0ull && (threadIdx.x & 63u) == 0u)
        (void) __hip_atomic_fetch_add(b + kSacPoison, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// caller order: the scan's input (1: an inlier of the returned plane) and the label
__global__ void __launch_bounds__(kBlock)
    k_sac_select(const float4 *__restrict__ pts, unsigned n, float4 pl, float thr, unsigned *__restrict__ flag,
                 unsigned char *__restrict__ labels) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const bool in = sac_dist(pl, p.x, p.y, p.z) < thr;
    flag[i] = in ? 1u : 0u;
    if (labels) labels[i] = (unsigned char) (in ? WM_SAC_INLIER : p.x == p.x ? WM_SAC_OUTLIER : WM_SAC_NONE);
}

// pos = the exclusive scan of flag (n + 1 entries): the inliers' indices ascending, the first `cap` of them
__global__ void __launch_bounds__(kBlock)
    k_sac_compact(const unsigned *__restrict__ flag, const unsigned *__restrict__ pos, unsigned n, unsigned cap,
                  int *__restrict__ idx_out) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const unsigned at = pos[i];
    if (at < cap) idx_out[at] = (int) i;
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

}  // namespace

// The context's workspace of the plane segmentation: its own buffers, shared with nothing else on the context.
struct SacWs {
    DevBuf pts;            // the packed cloud
    DevBuf round;          // a round: [R float4 planes][R flags][R counts][4 words: the finite points, the inliers]
    DevBuf bins;           // the refit's limbs + the tail (p0)
    DevBuf flag, pos;      // the selection's scan
    DevBuf idx, labels;    // host outputs on their way
    PinnedBuf h_round, h_bins;
};

void sac_release(wm_ctx *ctx) {
    SacWs *w = static_cast<SacWs *>(ctx->sac);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts, &w->round, &w->bins, &w->flag, &w->pos, &w->idx, &w->labels};
    for (DevBuf *b : bufs) b->release();
    w->h_round.release();
    w->h_bins.release();
    delete w;
    ctx->sac = nullptr;
}

namespace {

bool sac_args_ok(const wm_sac_params *p, size_t stride, int mem, int out_mem) {
    if (!p || stride < 12 || (stride & 3) || !(mem == WM_MEM_HOST || mem == WM_MEM_DEVICE) ||
        !(out_mem == WM_MEM_HOST || out_mem == WM_MEM_DEVICE))
        return false;
    if (!(p->model == WM_SAC_PLANE || p->model == WM_SAC_PERPENDICULAR_PLANE || p->model == WM_SAC_PARALLEL_PLANE)) return false;
    if (!std::isfinite(p->distance_threshold) || !(p->distance_threshold > 0) || p->max_iterations < 1 ||
        !(p->probability > 0 && p->probability < 1))
        return false;
    if (p->model != WM_SAC_PLANE) {
        const double n2 = (p->axis[0] * p->axis[0] + p->axis[1] * p->axis[1]) + p->axis[2] * p->axis[2];
        if (!std::isfinite(n2) || !(n2 > 0) || !(std::sqrt(n2) > 0)) return false;
        if (!(p->eps_angle > 0 && p->eps_angle <= 1.5707963267948966)) return false;
    }
    return true;
}

// PCL's bound on the iterations for an inlier fraction w
double sac_k(double log_p, double w) {
    double q = 1.0 - std::pow(w, 3.0);
    q = std::max(DBL_EPSILON, std::min(1.0 - DBL_EPSILON, q));
    return log_p / std::log(q);
}

// double -> float toward zero: the normal the refit returns is never longer than the unit eigenvector, so that its
// n' C n does not exceed the smallest eigenvalue by what a longer vector would add
float sac_toward_zero(double v) {
    float f = (float) v;
    if (std::fabs((double) f) > std::fabs(v)) f = nextafterf(f, 0.f);
    return f;
}

float sac_threshold(double t) {  // the smallest float not below t
    float f = (float) t;
    if ((double) f < t) f = nextafterf(f, INFINITY);
    return f;
}

// The plane of the sums (relative to p0): the eigenvector of the covariance's smallest eigenvalue, its sign the
// model's; false: not finite, the model stays.
bool sac_refit(const long long *bins, const float *p0, double m, const float model[4], float out[4]) {
    double sum[kSacComps];
    for (int c = 0; c < kSacComps; ++c) {
        double s = 0.0;
        for (int b = 0; b < kSacBins; ++b) {  // (a bin's limbs are exact integers: its value is a function of the inliers)
            const long long *w = bins + (size_t) b * (kBinLimbs * kSacStride) + c;
            s += bins_value(w[0], w[kSacStride], w[2 * kSacStride]);
        }
        sum[c] = s;
    }
    for (int b = 0; b < kSacBins; ++b)
        if (bins[(size_t) b * (kBinLimbs * kSacStride) + kSacPoison] != 0ll) return false;
    const double mx = sum[0] / m, my = sum[1] / m, mz = sum[2] / m;
    const double cxx = sum[3] / m - mx * mx, cxy = sum[4] / m - mx * my, cxz = sum[5] / m - mx * mz;
    const double cyy = sum[6] / m - my * my, cyz = sum[7] / m - my * mz, czz = sum[8] / m - mz * mz;
    const double C[9] = {cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz};
    for (double v : C)
        if (!std::isfinite(v)) return false;
    double U[9], S[3], V[9];
    svd3<false>(C, U, S, V);  // (symmetric, positive semi-definite: the right singular vectors are the eigenvectors)
    double nx = V[2], ny = V[5], nz = V[8];
    if ((nx * (double) model[0] + ny * (double) model[1]) + nz * (double) model[2] < 0) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    const float fx = sac_toward_zero(nx), fy = sac_toward_zero(ny), fz = sac_toward_zero(nz);
    // d = -n . centroid with the normal as it is returned
    const double gx = (double) p0[0] + mx, gy = (double) p0[1] + my, gz = (double) p0[2] + mz;
    const float fd = (float) -(((double) fx * gx + (double) fy * gy) + (double) fz * gz);
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(fz) && std::isfinite(fd))) return false;
    if (fx == 0.f && fy == 0.f && fz == 0.f) return false;
    out[0] = fx;
    out[1] = fy;
    out[2] = fz;
    out[3] = fd;
    return true;
}

int sac_run(wm_ctx *ctx, const void *pts_in, size_t n, size_t stride, int mem, const wm_sac_params *p, float *coef_out,
            int32_t *indices_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out, wm_sac_stats *stats) {
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->sac) ctx->sac = new SacWs();
    SacWs &w = *static_cast<SacWs *>(ctx->sac);
    hipStream_t st = ctx->stream;
    const bool host_out = out_mem == WM_MEM_HOST, timed = stats != nullptr;
    const unsigned nu = (unsigned) n;
    const unsigned Rmax = (unsigned) std::min(std::max(ctx->tune_sac_round, 1), kSacMaxRound);
    const float thr = sac_threshold(p->distance_threshold);
    SacAxis ax{p->model, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p->model != WM_SAC_PLANE) {
        const double l = std::sqrt((p->axis[0] * p->axis[0] + p->axis[1] * p->axis[1]) + p->axis[2] * p->axis[2]);
        ax.x = (float) (p->axis[0] / l);
        ax.y = (float) (p->axis[1] / l);
        ax.z = (float) (p->axis[2] / l);
        ax.cos_eps = (float) std::cos(p->eps_angle);
        ax.sin_eps = (float) std::sin(p->eps_angle);
    }

    // a round's record: the planes, the flags, the counts, four words of results
    const size_t round_bytes = (size_t) Rmax * (sizeof(float4) + 8) + 16;
    WM_HIP(ctx, w.pts.reserve(n * sizeof(float4)));
    WM_HIP(ctx, w.round.reserve(round_bytes));
    WM_HIP(ctx, w.h_round.reserve(round_bytes));
    float4 *d_pts = w.pts.as<float4>();
    float4 *d_planes = w.round.as<float4>();
    unsigned *d_flags = reinterpret_cast<unsigned *>(d_planes + Rmax), *d_counts = d_flags + Rmax, *d_res = d_counts + Rmax;
    const float4 *h_planes = w.h_round.as<float4>();
    const unsigned *h_flags = reinterpret_cast<const unsigned *>(h_planes + Rmax), *h_counts = h_flags + Rmax,
                   *h_res = h_counts + Rmax;

    if (timed) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    WM_TRY(pack_cloud(ctx, pts_in, n, stride, mem, d_pts));
    WM_HIP(ctx, hipMemsetAsync(d_res, 0, 16, st));
    const unsigned count_blocks = (unsigned) std::min<size_t>((n + kSacTile - 1) / kSacTile, kSacMaxBlocks);

    // ---- PCL's loop over the stream, a round at a time
    const double log_p = std::log(1.0 - p->probability);
    const long long max_it = p->max_iterations, max_skip = 10ll * max_it;
    long long it = 0, skipped = 0, best = -1, best_j = -1;
    unsigned long long j = 0;  // the next stream entry
    double k = 1.0;
    float model[4] = {0.f, 0.f, 0.f, 0.f};
    int rounds = 0;
    size_t n_finite = 0;
    bool going = (double) it < k && skipped < max_skip;
    while (going) {
        const unsigned R = (unsigned) std::min<long long>(Rmax, max_it + 1 - it);
        hipLaunchKernelGGL(k_sac_hypotheses, dim3(blocks_of(R)), dim3(kBlock), 0, st, (const float4 *) d_pts, nu,
                           (unsigned long long) p->seed, j, R, ax, d_planes, d_flags, d_counts);
        hipLaunchKernelGGL(k_sac_count, dim3(count_blocks), dim3(kBlock), 0, st, (const float4 *) d_pts, nu,
                           (const float4 *) d_planes, (const unsigned *) d_flags, R, thr, d_counts,
                           rounds == 0 ? d_res : (unsigned *) nullptr);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(fast_fetch(ctx, w.h_round.p, w.round.p, round_bytes));
        if (rounds == 0) n_finite = h_res[0];
        ++rounds;
        for (unsigned e = 0; e < R && going; ++e, ++j) {
            if (h_flags[e] == kSacSkipped) {
                ++skipped;
            } else {
                const long long c = (long long) h_counts[e];
                if (h_flags[e] == kSacValid && c > best) {
                    best = c;
                    best_j = (long long) j;
                    memcpy(model, &h_planes[e], sizeof(model));
                    k = sac_k(log_p, (double) c / (double) n);
                } else if (h_flags[e] == kSacAxisInvalid && best < 0) {
                    k = sac_k(log_p, 0.0);  // (PCL: its count of 0 beats "nothing counted yet" and sets k; it is no model)
                }
                ++it;
                if (it > max_it) {
                    ++j;
                    going = false;
                    break;
                }
            }
            going = (double) it < k && skipped < max_skip;
        }
    }
    if (stats) {
        stats->n_finite = n_finite;
        stats->iterations = (int) it;
        stats->skipped = (int) skipped;
        stats->rounds = rounds;
        stats->hypotheses = (long long) j;
        stats->best_hypothesis = best_j;
    }
    auto finish_timing = [&]() {
        if (!timed) return;
        (void) hipEventRecord(ctx->ev_b, st);
        (void) hipStreamSynchronize(st);
        float ms = 0.f;
        (void) hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b);
        stats->kernel_ms = ms;
    };
    if (best_j < 0) {
        finish_timing();
        return WM_NOT_CONVERGED;
    }
    if (stats) {
        stats->n_inliers_model = (size_t) best;
        memcpy(stats->model_coefficients, model, sizeof(model));
    }

    // ---- the refit
    float coef[4] = {model[0], model[1], model[2], model[3]};
    int refined = 0;
    if (p->optimize_coefficients && best >= 4) {
        unsigned s[3];
        sac_sample((unsigned long long) p->seed, (unsigned long long) best_j, nu, s);
        const size_t bins_bytes = kSacBinWords * sizeof(long long) + sizeof(float4);
        WM_HIP(ctx, w.bins.reserve(bins_bytes));
        WM_HIP(ctx, w.h_bins.reserve(bins_bytes));
        long long *d_bins = w.bins.as<long long>();
        WM_HIP(ctx, hipMemsetAsync(d_bins, 0, bins_bytes, st));
        hipLaunchKernelGGL(k_sac_sums, dim3(blocks_of(n)), dim3(kBlock), 0, st, (const float4 *) d_pts, nu,
                           make_float4(model[0], model[1], model[2], model[3]), thr, s[0], d_bins,
                           reinterpret_cast<float4 *>(d_bins + kSacBinWords));
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(fast_fetch(ctx, w.h_bins.p, w.bins.p, bins_bytes));
        const long long *h_bins = w.h_bins.as<long long>();
        if (sac_refit(h_bins, reinterpret_cast<const float *>(h_bins + kSacBinWords), (double) best, model, coef)) refined = 1;
        else memcpy(coef, model, sizeof(coef));
    }

    // ---- the selection with the returned coefficients
    WM_HIP(ctx, w.flag.reserve(n * 4));
    WM_HIP(ctx, w.pos.reserve((n + 1) * 4));
    unsigned char *d_labels = labels_out;
    if (labels_out && host_out) {
        WM_HIP(ctx, w.labels.reserve(n));
        d_labels = w.labels.as<unsigned char>();
    }
    int *d_idx = indices_out;
    if (host_out && cap > 0) {
        WM_HIP(ctx, w.idx.reserve(std::min(cap, n) * 4));
        d_idx = w.idx.as<int>();
    }
    unsigned *flag = w.flag.as<unsigned>(), *pos = w.pos.as<unsigned>();
    hipLaunchKernelGGL(k_sac_select, dim3(blocks_of(n)), dim3(kBlock), 0, st, (const float4 *) d_pts, nu,
                       make_float4(coef[0], coef[1], coef[2], coef[3]), thr, flag, d_labels);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, flag, n, pos));
    if (cap > 0) {
        hipLaunchKernelGGL(k_sac_compact, dim3(blocks_of(n)), dim3(kBlock), 0, st, (const unsigned *) flag, (const unsigned *) pos,
                           nu, (unsigned) std::min(cap, n), d_idx);
        WM_HIP(ctx, hipGetLastError());
    }
    WM_TRY(fast_fetch(ctx, w.h_round.p, pos + n, 4));
    const size_t n_in = *w.h_round.as<unsigned>();
    finish_timing();
    WM_HIP(ctx, hipStreamSynchronize(st));
    const size_t n_idx = std::min(n_in, cap);
    if (host_out) {
        if (n_idx) WM_HIP(ctx, hipMemcpy(indices_out, d_idx, n_idx * 4, hipMemcpyDeviceToHost));
        if (labels_out) WM_HIP(ctx, hipMemcpy(labels_out, d_labels, n, hipMemcpyDeviceToHost));
    }
    memcpy(coef_out, coef, sizeof(coef));
    *n_out = n_in;
    if (stats) {
        stats->n_inliers = n_in;
        stats->refined = refined;
    }
    return n_in > cap ? WM_ERR_ARG : WM_OK;
}

}  // namespace

}  // namespace wm

using namespace wm;

extern "C" {

void wm_sac_default_params(wm_sac_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->model = WM_SAC_PLANE;  // sac_segmentation.h: threshold_ (0), max_iterations_ (50), probability_ (0.99), optimize_coefficients_ (true)
    p->distance_threshold = 0.0;
    p->max_iterations = 50;
    p->probability = 0.99;
    p->optimize_coefficients = 1;
    p->seed = 0;
}

int wm_sac_segment(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_sac_params *p,
                   float coefficients_out[4], int32_t *indices_out, size_t cap, int out_mem, size_t *n_out,
                   uint8_t *labels_out, wm_sac_stats *stats) {
    if (!ctx || !n_out || !coefficients_out || (n > 0 && !pts) || n > 0x7FFFFFF0u || (cap > 0 && !indices_out) ||
        !sac_args_ok(p, stride, mem, out_mem))
        return WM_ERR_ARG;
    *n_out = 0;
    if (stats) {
        *stats = wm_sac_stats{};
        stats->best_hypothesis = -1;
    }
    if (n < 3) return WM_NOT_CONVERGED;  // (no sample: no device is touched)
    return sac_run(ctx, pts, n, stride, mem, p, coefficients_out, indices_out, cap, out_mem, n_out, labels_out, stats);
}

}  // extern "C"
