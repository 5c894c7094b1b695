// wm_corr_ransac.hip -- a pose from correspondences on the device: pcl::registration::CorrespondenceRejectorSample-
// Consensus as one call (wm_corr_ransac), the stage behind wm_fpfh_estimate and wm_feature_match.  RANSAC over the
// correspondences with a rigid transform from three pairs; the hot loop is hypotheses x pairs transform tests.
//
// The rule is stated in include/wavematch.h ("pose from correspondences"); what of it is evaluated in more than one
// place is wm_corr_rule.hpp, for host and device alike; the checker is tests/corr_ransac_reference.py.  The hypothesis
// stream is the plane segmentation's (wm_sac.hip): a function of (seed, j, mv), evaluated in ROUNDS of up to
// `corr_round` entries, whose (flag, count) pairs the host walks in stream order with PCL's loop (SacWalk,
// wm_sac_walk.hpp).  A round never holds more entries than the loop can still count as iterations.  How the stream is
// cut into rounds changes no output but `rounds`.
//   front      k_corr_flag (an entry is valid: both indices in range, both points finite) -> exclusive_scan ->
//              k_corr_gather: pair i as two float4 (p, q) in pair order and its entry e.  The hot kernel then reads 32
//              contiguous bytes per pair and no index.  With the automatic sample distance: k_corr_sums<kCov> and
//              k_corr_bins_sums, the nine sums of the pairs' source points as exact integer limbs (wm_bins.hpp's
//              splitting).  One fetch of the CorrHead: mv and the sums
//   a round    k_corr_hypotheses   one lane per stream entry: the sample, six float4 loads, the rule (a 3 x 3 Umeyama
//                                  step in double with IEEE divisions and square roots); twelve floats in three float4,
//                                  a flag and a zero count
//              k_corr_count        the hot kernel.  A lane keeps kCorrPts pairs in registers and loops over the
//                                  round's transforms, read through a wave-uniform index (scalar loads), the next
//                                  one's loads issued before this one's tests; per transform a ballot and a popcount per
//                                  pair slot, accumulated per workgroup in LDS; ONE integer atomicAdd per transform and
//                                  workgroup at its end.  Integer counts: order-independent
//              one fetch of the round's (flag, count) pairs, 8 bytes an entry
//   behind     k_corr_model        a lane: the model is entry best_j of the stream, evaluated again, with its sample's
//                                  first pair (p0, q0)
//              the refit           k_corr_sums<kRefit> and k_corr_bins_sums: the fifteen sums of the model's inliers
//                                  relative to (p0, q0), exact; one fetch; Umeyama on the host
//              k_corr_select (flags and labels) -> exclusive_scan -> k_corr_compact, one fetch of the CorrHead
// Host waits: the front 1, R rounds, the end 1, + 1 with the refit (the automatic sample distance rides in the front's).
#include <float.h>
#include <string.h>

#include "wm_bins.hpp"
#include "wm_corr_rule.hpp"
#include "wm_sac_walk.hpp"

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

constexpr int kCorrMaxRound = 1024;             // the option's upper end: s_cnt of the count kernel
constexpr int kCorrPts = 4;                     // pairs a lane of the count kernel keeps in registers (24 floats)
constexpr int kCorrTile = kBlock * kCorrPts;    // pairs of a workgroup's tile
constexpr unsigned kCorrMaxBlocks = 2048;       // count workgroups at the most (8 per CU): each walks tiles
// the sums' bins: kCorrBins bins x kBinLimbs limb rows x kCorrStride words; components 0 ... 14 in use at the most, word
// kCorrPoison of limb row 0 counts terms the limbs cannot hold.  A limb of one addend is below 2^40, a bin's word holds
// 2^63 and a call has at most 2^20 pairs.
constexpr int kCorrBins = 64;
constexpr int kCorrStride = 16;
constexpr int kCorrPoison = kCorrStride - 1;
constexpr int kCorrBinSize = kBinLimbs * kCorrStride;
constexpr int kCovComps = 9;
enum { kCov = 0, kRefit = 1 };

// ------------------------------------------------------------------ the hypothesis stream (wm_sac.hip's, bit for bit)
WM_HD unsigned long long corr_sm64(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
WM_HD unsigned corr_r(unsigned long long seed, unsigned long long j, unsigned a, unsigned m) {
    const unsigned long long h = corr_sm64(seed + 0x9E3779B97F4A7C15ull * (3ull * j + a + 1ull));
    return (unsigned) (((h >> 32) * (unsigned long long) m) >> 32);
}
// (n >= 3)
WM_HD void corr_sample(unsigned long long seed, unsigned long long j, unsigned n, unsigned (&i)[3]) {
    i[0] = corr_r(seed, j, 0u, n);
    unsigned t = corr_r(seed, j, 1u, n - 1u);
    i[1] = t + (t >= i[0] ? 1u : 0u);
    const unsigned lo = i[0] < i[1] ? i[0] : i[1], hi = i[0] < i[1] ? i[1] : i[0];
    t = corr_r(seed, j, 2u, n - 2u);
    t += t >= lo ? 1u : 0u;
    t += t >= hi ? 1u : 0u;
    i[2] = t;
}

// What the host needs of the front and of the end, in one small fetch.
struct CorrHead {
    double sum[16];   // the front's nine sums, later the refit's fifteen
    float model[12];  // k_corr_model: the winning entry's transform
    float p0[4], q0[4];  // ... and its sample's first pair
    unsigned poison, mv, n_out, pad;
};

// ------------------------------------------------------------------ the front
// flag[e] = entry e is valid.  The clouds are the caller's records (x y z first).
__global__ void __launch_bounds__(kBlock)
    k_corr_flag(const unsigned char *__restrict__ src, unsigned n_src, const unsigned char *__restrict__ tgt, unsigned n_tgt,
                size_t stride, const int *__restrict__ qidx, const int *__restrict__ midx, unsigned m,
                unsigned *__restrict__ flag) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= m) return;
    const long long si = qidx ? (long long) qidx[e] : (long long) e, ti = midx[e];
    unsigned ok = 0u;
    if (si >= 0 && si < (long long) n_src && ti >= 0 && ti < (long long) n_tgt) {
        const float *p = reinterpret_cast<const float *>(src + (size_t) si * stride);
        const float *q = reinterpret_cast<const float *>(tgt + (size_t) ti * stride);
        ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) ? 1u : 0u;
    }
    flag[e] = ok;
}

// pos = the exclusive scan of flag (m + 1 entries).  Pair pos[e] of a valid entry e: its points and e.
__global__ void __launch_bounds__(kBlock)
    k_corr_gather(const unsigned char *__restrict__ src, const unsigned char *__restrict__ tgt, size_t stride,
                  const int *__restrict__ qidx, const int *__restrict__ midx, unsigned m, const unsigned *__restrict__ flag,
                  const unsigned *__restrict__ pos, float4 *__restrict__ pairs, int *__restrict__ pair_e,
                  CorrHead *__restrict__ head) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e == 0u) {
        head->mv = pos[m];
        head->poison = 0u;
        head->n_out = 0u;
    }
    if (e >= m || !flag[e]) return;
    const size_t si = qidx ? (size_t) qidx[e] : (size_t) e, ti = (size_t) midx[e];  // (in range: the entry is valid)
    const float *p = reinterpret_cast<const float *>(src + si * stride);
    const float *q = reinterpret_cast<const float *>(tgt + ti * stride);
    const unsigned at = pos[e];
    pairs[2 * (size_t) at] = make_float4(p[0], p[1], p[2], 0.f);
    pairs[2 * (size_t) at + 1] = make_float4(q[0], q[1], q[2], 0.f);
    pair_e[at] = (int) e;
}

// ------------------------------------------------------------------ a round
__device__ __forceinline__ unsigned corr_entry(const float4 *__restrict__ pairs, unsigned mv, unsigned long long seed,
                                               unsigned long long j, float min_d2, float (&T)[12], float4 *p0, float4 *q0) {
    unsigned i[3];
    corr_sample(seed, j, mv, i);  // (each index < mv by construction)
    float p[9], q[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 a = pairs[2 * (size_t) i[k]], b = pairs[2 * (size_t) i[k] + 1];
        p[3 * k] = a.x;
        p[3 * k + 1] = a.y;
        p[3 * k + 2] = a.z;
        q[3 * k] = b.x;
        q[3 * k + 1] = b.y;
        q[3 * k + 2] = b.z;
        if (k == 0) {
            if (p0) *p0 = a;
            if (q0) *q0 = b;
        }
    }
    return corr_hypothesis(p, q, min_d2, T);
}

// One lane per entry of the round.  counts[e] = 0 for the count kernel behind it.
__global__ void __launch_bounds__(kBlock)
    k_corr_hypotheses(const float4 *__restrict__ pairs, unsigned mv, unsigned long long seed, unsigned long long j0, unsigned R,
                      float min_d2, float4 *__restrict__ T3, unsigned *__restrict__ flags, unsigned *__restrict__ counts) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= R) return;
    float T[12];
    const unsigned flag = corr_entry(pairs, mv, seed, j0 + e, min_d2, T, nullptr, nullptr);
    T3[3 * e] = make_float4(T[0], T[1], T[2], T[3]);
    T3[3 * e + 1] = make_float4(T[4], T[5], T[6], T[7]);
    T3[3 * e + 2] = make_float4(T[8], T[9], T[10], T[11]);
    flags[e] = flag;
    if (counts) counts[e] = 0u;
}

__device__ __forceinline__ float corr_d2(const float4 &r0, const float4 &r1, const float4 &r2, float x, float y, float z,
                                         float qx, float qy, float qz) {
    const float T[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
    return corr_pair_d2(T, x, y, z, qx, qy, qz);
}

// The hot kernel.  The workgroup walks tiles of kCorrTile pairs; of a tile a lane holds kCorrPts pairs (slot u: pair
// tile * kCorrTile + u * kBlock + thread, coalesced) and tests them against every valid transform of the round.  A slot
// behind the last pair holds NaN and fails d2 < thr2.
__global__ void __launch_bounds__(kBlock)
    k_corr_count(const float4 *__restrict__ pairs, unsigned mv, const float4 *__restrict__ T3, const unsigned *__restrict__ flags,
                 unsigned R, float thr2, unsigned *__restrict__ counts) {
    __shared__ unsigned s_cnt[kCorrMaxRound];
    for (unsigned j = threadIdx.x; j < R; j += kBlock) s_cnt[j] = 0u;
    __syncthreads();
    const bool lane0 = (threadIdx.x & 63u) == 0u;
    const float nanv = __builtin_nanf("");
    for (size_t t0 = (size_t) blockIdx.x * kCorrTile; t0 < mv; t0 += (size_t) gridDim.x * kCorrTile) {
        float x[kCorrPts], y[kCorrPts], z[kCorrPts], qx[kCorrPts], qy[kCorrPts], qz[kCorrPts];
#pragma unroll
        for (int u = 0; u < kCorrPts; ++u) {
            const size_t i = t0 + (size_t) u * kBlock + threadIdx.x;
            x[u] = y[u] = z[u] = qx[u] = qy[u] = qz[u] = nanv;
            if (i < mv) {
                const float4 p = pairs[2 * i], q = pairs[2 * i + 1];
                x[u] = p.x;
                y[u] = p.y;
                z[u] = p.z;
                qx[u] = q.x;
                qy[u] = q.y;
                qz[u] = q.z;
            }
        }
        float4 a_next = T3[0], b_next = T3[1], c_next = T3[2];  // (R >= 1) the next transform's scalar loads run under this one's tests
        unsigned flag_next = flags[0];
        for (unsigned j = 0; j < R; ++j) {
            const float4 a = a_next, b = b_next, c = c_next;
            const unsigned flag = flag_next;
            const unsigned jn = j + 1u < R ? j + 1u : j;
            a_next = T3[3 * jn];
            b_next = T3[3 * jn + 1];
            c_next = T3[3 * jn + 2];
            flag_next = flags[jn];
            if (flag != kCorrValid) continue;  // (the same for every lane)
            unsigned n = 0u;
#pragma unroll
            for (int u = 0; u < kCorrPts; ++u)
                n += (unsigned) __popcll(__ballot(corr_d2(a, b, c, x[u], y[u], z[u], qx[u], qy[u], qz[u]) < thr2));
            if (lane0 && n) atomicAdd(&s_cnt[j], n);
        }
    }
    __syncthreads();
    for (unsigned j = threadIdx.x; j < R; j += kBlock)
        if (s_cnt[j]) atomicAdd(&counts[j], s_cnt[j]);
}

// ------------------------------------------------------------------ behind the rounds
// One lane: the model is entry best_j of the stream, evaluated again; (p0, q0) its sample's first pair.
__global__ void k_corr_model(const float4 *__restrict__ pairs, unsigned mv, unsigned long long seed, unsigned long long best_j,
                             float min_d2, CorrHead *__restrict__ head) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    float T[12];
    float4 p0, q0;
    (void) corr_entry(pairs, mv, seed, best_j, min_d2, T, &p0, &q0);
#pragma unroll
    for (int k = 0; k < 12; ++k) head->model[k] = T[k];
    head->p0[0] = p0.x;
    head->p0[1] = p0.y;
    head->p0[2] = p0.z;
    head->p0[3] = 0.f;
    head->q0[0] = q0.x;
    head->q0[1] = q0.y;
    head->q0[2] = q0.z;
    head->q0[3] = 0.f;
}

// A wave's share of NC sums into bin b: each lane's terms (zero where the lane has none) are split into limbs
// (bins_split: a function of the term alone); the limbs are integers, so the wave's shuffles and the bin's atomics add
// them exactly in any order.  Called by every lane of the wave.
template <int NC>
__device__ __forceinline__ void corr_sums_wave(bool in, const double (&term)[NC], long long *__restrict__ b) {
    if (__ballot(in) == 0ull) return;  // (the whole wave)
    bool poison = false;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        long long l[kBinLimbs] = {0ll, 0ll, 0ll};
        if (fabs(term[c]) < 4611686018427387904.0) bins_split(term[c], l);  // (2^62)
        else poison = true;
#pragma unroll
        for (int k = 0; k < kBinLimbs; ++k) {
            long long v = l[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if ((threadIdx.x & 63u) == 0u && v != 0ll)
                (void) __hip_atomic_fetch_add(b + k * kCorrStride + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (__ballot(poison) != 0ull && (threadIdx.x & 63u) == 0u)
        (void) __hip_atomic_fetch_add(b + kCorrPoison, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// kCov: the nine sums of every pair's source point relative to pair 0's.  kRefit: the fifteen sums of the model's
// inliers relative to (p0, q0).  The grid covers `cover` >= mv pairs (the front does not know mv yet: head->mv).
template <int MODE>
__global__ void __launch_bounds__(kBlock)
    k_corr_sums(const float4 *__restrict__ pairs, const CorrHead *__restrict__ head, float thr2, long long *__restrict__ bins) {
    const unsigned mv = head->mv;
    if (blockIdx.x * kBlock >= mv) return;  // (the whole workgroup)
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    const unsigned wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    long long *b = bins + (size_t) (wave % kCorrBins) * kCorrBinSize;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = p;
    bool in = i < mv;
    if (in) {
        p = pairs[2 * (size_t) i];
        q = pairs[2 * (size_t) i + 1];
    }
    if (MODE == kCov) {
        const float4 o = pairs[0];
        const double dx = in ? (double) p.x - (double) o.x : 0.0, dy = in ? (double) p.y - (double) o.y : 0.0,
                     dz = in ? (double) p.z - (double) o.z : 0.0;
        const double term[kCovComps] = {dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
        corr_sums_wave<kCovComps>(in, term, b);
    } else {
        in = in && corr_pair_d2(head->model, p.x, p.y, p.z, q.x, q.y, q.z) < thr2;
        const double px = in ? (double) p.x - (double) head->p0[0] : 0.0, py = in ? (double) p.y - (double) head->p0[1] : 0.0,
                     pz = in ? (double) p.z - (double) head->p0[2] : 0.0;
        const double qx = in ? (double) q.x - (double) head->q0[0] : 0.0, qy = in ? (double) q.y - (double) head->q0[1] : 0.0,
                     qz = in ? (double) q.z - (double) head->q0[2] : 0.0;
        const double term[kCorrRefitComps] = {px, py, pz, qx, qy, qz, qx * px, qx * py, qx * pz,
                                              qy * px, qy * py, qy * pz, qz * px, qz * py, qz * pz};
        corr_sums_wave<kCorrRefitComps>(in, term, b);
    }
}

// One wave: thread c adds component c's limbs over the bins as integers (exact, any order) and turns the three totals
// into their double (bins_value): a sum is a function of the set of its terms.
__global__ void __launch_bounds__(64) k_corr_bins_sums(const long long *__restrict__ bins, int nc, CorrHead *__restrict__ head) {
    const int c = (int) threadIdx.x;
    if (c < nc) {
        long long L[kBinLimbs] = {0ll, 0ll, 0ll};
        for (int b = 0; b < kCorrBins; ++b)
#pragma unroll
            for (int k = 0; k < kBinLimbs; ++k) L[k] += bins[(size_t) b * kCorrBinSize + k * kCorrStride + c];
        head->sum[c] = bins_value(L[0], L[1], L[2]);
    }
    if (c == kCorrPoison) {
        unsigned poison = 0u;
        for (int b = 0; b < kCorrBins; ++b)
            if (bins[(size_t) b * kCorrBinSize + kCorrPoison] != 0ll) poison = 1u;
        head->poison = poison;
    }
}

struct CorrT {  // the returned transform's float rounding by value (has), else the model where k_corr_model left it
    int has;
    float T[12];
};

// flag[i] = pair i is an inlier of the returned transform; labels by entry (the invalid entries' are zero already).
__global__ void __launch_bounds__(kBlock)
    k_corr_select(const float4 *__restrict__ pairs, const int *__restrict__ pair_e, unsigned mv, CorrT t,
                  const CorrHead *__restrict__ head, float thr2, unsigned *__restrict__ flag, unsigned char *__restrict__ labels) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= mv) return;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = t.has ? t.T[k] : head->model[k];
    const float4 p = pairs[2 * (size_t) i], q = pairs[2 * (size_t) i + 1];
    const bool in = corr_pair_d2(T, p.x, p.y, p.z, q.x, q.y, q.z) < thr2;
    flag[i] = in ? 1u : 0u;
    if (labels) labels[pair_e[i]] = (unsigned char) (in ? WM_CORR_INLIER : WM_CORR_OUTLIER);
}

// pos = the exclusive scan of flag (mv + 1 entries): the kept pairs' entries, ascending.
__global__ void __launch_bounds__(kBlock)
    k_corr_compact(const int *__restrict__ pair_e, const unsigned *__restrict__ flag, const unsigned *__restrict__ pos, unsigned mv,
                   int *__restrict__ idx_out, size_t cap, CorrHead *__restrict__ head) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u) head->n_out = pos[mv];
    if (i >= mv || !flag[i]) return;
    const unsigned at = pos[i];
    if (at < cap) idx_out[at] = pair_e[i];
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

}  // namespace

// The context's workspace of the RANSAC over correspondences: its own buffers, shared with nothing else on the context.
struct CorrWs {
    DevBuf src, tgt, qidx, midx;  // a caller's host arrays on their way
    DevBuf flag, pos;             // the two scans (entries, then pairs)
    DevBuf pairs, pair_e;         // [2 mv] float4, [mv] entries
    DevBuf round;                 // [R flags][R counts] ... [3 R float4]
    DevBuf bins, head;
    DevBuf idx, labels;           // host outputs on their way
    PinnedBuf h_round, h_head;
    // what wm_debug_corr_hypotheses evaluates: the last call's pairs
    unsigned mv = 0;
    unsigned long long seed = 0;
    float min_d2 = 0.f;
    bool have = false;
};

void corr_release(wm_ctx *ctx) {
    CorrWs *w = static_cast<CorrWs *>(ctx->corr);
    if (!w) return;
    DevBuf *bufs[] = {&w->src, &w->tgt, &w->qidx, &w->midx, &w->flag, &w->pos, &w->pairs, &w->pair_e, &w->round, &w->bins,
                      &w->head, &w->idx, &w->labels};
    for (DevBuf *b : bufs) b->release();
    w->h_round.release();
    w->h_head.release();
    delete w;
    ctx->corr = nullptr;
}

namespace {

bool corr_params_ok(const wm_corr_ransac_params *p) {
    return p && std::isfinite(p->inlier_threshold) && p->inlier_threshold > 0 && p->max_iterations >= 1 &&
           p->probability > 0 && p->probability < 1 && std::isfinite(p->min_sample_distance);
}

unsigned corr_round_max(const wm_ctx *ctx) { return (unsigned) std::min(std::max(ctx->tune_corr_round, 1), kCorrMaxRound); }

// the round's words: [Rmax flags][Rmax counts], the transforms behind them at a float4's alignment
size_t corr_T3_at(unsigned Rmax) { return ((size_t) 2 * Rmax + 3) & ~(size_t) 3; }  // (words)
size_t corr_round_bytes(unsigned Rmax) { return corr_T3_at(Rmax) * 4 + (size_t) 3 * Rmax * sizeof(float4); }

struct CorrCall {
    const void *src;
    size_t n_src;
    const void *tgt;
    size_t n_tgt, stride;
    const int32_t *qidx, *midx;
    size_t m;
    int mem;
    const wm_corr_ransac_params *p;
    double *T_out;
    int32_t *inliers_out;
    size_t cap;
    bool host_out;
    size_t *n_out;
    uint8_t *labels_out;
    wm_corr_ransac_stats *stats;
};

// The call (arguments checked, the outputs' defaults written, m >= 3).
int corr_call(wm_ctx *ctx, const CorrCall &c) {
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->corr) ctx->corr = new CorrWs();
    CorrWs &w = *static_cast<CorrWs *>(ctx->corr);
    hipStream_t st = ctx->stream;
    const wm_corr_ransac_params *p = c.p;
    const unsigned m = (unsigned) c.m, Rmax = corr_round_max(ctx);
    const float thr2 = sac_threshold(p->inlier_threshold * p->inlier_threshold);
    const unsigned long long seed = (unsigned long long) p->seed;
    const bool timed = c.stats != nullptr, automatic = p->min_sample_distance < 0;
    w.have = false;

    WM_HIP(ctx, w.flag.reserve((size_t) m * 4));
    WM_HIP(ctx, w.pos.reserve(((size_t) m + 1) * 4));
    WM_HIP(ctx, w.pairs.reserve((size_t) 2 * m * sizeof(float4)));
    WM_HIP(ctx, w.pair_e.reserve((size_t) m * 4));
    WM_HIP(ctx, w.round.reserve(corr_round_bytes(Rmax)));
    WM_HIP(ctx, w.bins.reserve((size_t) kCorrBins * kCorrBinSize * sizeof(long long)));
    WM_HIP(ctx, w.head.reserve(sizeof(CorrHead)));
    WM_HIP(ctx, w.h_round.reserve((size_t) 2 * Rmax * 4));
    WM_HIP(ctx, w.h_head.reserve(sizeof(CorrHead)));
    // ---- the inputs: where they are in device memory, else up into the workspace (the caller's pages: blocking copies)
    const unsigned char *d_src = static_cast<const unsigned char *>(c.src), *d_tgt = static_cast<const unsigned char *>(c.tgt);
    const int *d_q = c.qidx, *d_m = c.midx;
    if (c.mem == WM_MEM_HOST) {
        WM_HIP(ctx, hipStreamSynchronize(st));  // (a previous call may still read the workspace)
        WM_HIP(ctx, w.src.reserve(c.n_src * c.stride));
        WM_HIP(ctx, w.tgt.reserve(c.n_tgt * c.stride));
        WM_HIP(ctx, w.midx.reserve((size_t) m * 4));
        WM_HIP(ctx, hipMemcpy(w.src.p, c.src, c.n_src * c.stride, hipMemcpyHostToDevice));
        WM_HIP(ctx, hipMemcpy(w.tgt.p, c.tgt, c.n_tgt * c.stride, hipMemcpyHostToDevice));
        WM_HIP(ctx, hipMemcpy(w.midx.p, c.midx, (size_t) m * 4, hipMemcpyHostToDevice));
        d_src = w.src.as<unsigned char>();
        d_tgt = w.tgt.as<unsigned char>();
        d_m = w.midx.as<int>();
        if (c.qidx) {
            WM_HIP(ctx, w.qidx.reserve((size_t) m * 4));
            WM_HIP(ctx, hipMemcpy(w.qidx.p, c.qidx, (size_t) m * 4, hipMemcpyHostToDevice));
            d_q = w.qidx.as<int>();
        }
    }
    unsigned *flag = w.flag.as<unsigned>(), *pos = w.pos.as<unsigned>();
    float4 *pairs = w.pairs.as<float4>();
    int *pair_e = w.pair_e.as<int>();
    CorrHead *d_head = w.head.as<CorrHead>();
    const CorrHead *h_head = w.h_head.as<CorrHead>();
    long long *d_bins = w.bins.as<long long>();
    const size_t bins_bytes = (size_t) kCorrBins * kCorrBinSize * sizeof(long long);

    // ---- the front
    if (timed) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    hipLaunchKernelGGL(k_corr_flag, dim3(blocks_of(m)), dim3(kBlock), 0, st, d_src, (unsigned) c.n_src, d_tgt, (unsigned) c.n_tgt,
                       c.stride, d_q, d_m, m, flag);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, flag, m, pos));
    hipLaunchKernelGGL(k_corr_gather, dim3(blocks_of(m)), dim3(kBlock), 0, st, d_src, d_tgt, c.stride, d_q, d_m, m,
                       (const unsigned *) flag, (const unsigned *) pos, pairs, pair_e, d_head);
    if (automatic) {
        WM_HIP(ctx, hipMemsetAsync(d_bins, 0, bins_bytes, st));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_corr_sums<kCov>), dim3(blocks_of(m)), dim3(kBlock), 0, st, (const float4 *) pairs,
                           (const CorrHead *) d_head, thr2, d_bins);
        hipLaunchKernelGGL(k_corr_bins_sums, dim3(1), dim3(64), 0, st, (const long long *) d_bins, kCovComps, d_head);
    }
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(fast_fetch(ctx, w.h_head.p, d_head, sizeof(CorrHead)));
    const unsigned mv = h_head->mv;
    if (c.stats) c.stats->n_valid = mv;
    auto no_model = [&]() -> int {
        if (timed) {
            WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
            WM_HIP(ctx, hipStreamSynchronize(st));
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b) != hipSuccess) ms = 0.f;
            c.stats->kernel_ms = ms;
        }
        return WM_NOT_CONVERGED;
    };
    if (mv < 3) return no_model();
    const float min_d2 = automatic ? corr_min_d2_from_sums(h_head->sum, h_head->poison != 0u, (double) mv)
                                   : corr_min_d2_given(p->min_sample_distance);
    if (c.stats) c.stats->min_d2 = min_d2;
    w.mv = mv;
    w.seed = seed;
    w.min_d2 = min_d2;
    w.have = true;

    // ---- the rounds
    unsigned *d_words = w.round.as<unsigned>();
    float4 *d_T3 = reinterpret_cast<float4 *>(d_words + corr_T3_at(Rmax));
    const unsigned *h_words = w.h_round.as<unsigned>();
    const unsigned count_blocks = (unsigned) std::min<size_t>(((size_t) mv + kCorrTile - 1) / kCorrTile, kCorrMaxBlocks);
    SacWalk walk;
    walk.start(p->max_iterations, p->probability, mv);
    while (walk.going) {
        const unsigned R = walk.round_size(Rmax);
        unsigned *d_flags = d_words, *d_counts = d_words + R;
        hipLaunchKernelGGL(k_corr_hypotheses, dim3(blocks_of(R)), dim3(kBlock), 0, st, (const float4 *) pairs, mv, seed,
                           (unsigned long long) walk.j, R, min_d2, d_T3, d_flags, d_counts);
        hipLaunchKernelGGL(k_corr_count, dim3(count_blocks), dim3(kBlock), 0, st, (const float4 *) pairs, mv, (const float4 *) d_T3,
                           (const unsigned *) d_flags, R, thr2, d_counts);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(fast_fetch(ctx, w.h_round.p, d_words, (size_t) 2 * R * 4));
        walk.feed_round(h_words, h_words + R, R);
    }
    if (c.stats) {
        c.stats->iterations = (int) walk.it;
        c.stats->skipped = (int) walk.skipped;
        c.stats->rounds = walk.rounds;
        c.stats->hypotheses = (long long) walk.j;
        c.stats->best_hypothesis = walk.best_j;
    }
    if (walk.best_j < 0) return no_model();

    // ---- the model again from its entry; the refit
    hipLaunchKernelGGL(k_corr_model, dim3(1), dim3(64), 0, st, (const float4 *) pairs, mv, seed, (unsigned long long) walk.best_j,
                       min_d2, d_head);
    CorrT t{};
    double T[16];
    bool refined = false;
    if (p->refine_model && walk.best >= 3) {
        WM_HIP(ctx, hipMemsetAsync(d_bins, 0, bins_bytes, st));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_corr_sums<kRefit>), dim3(blocks_of(mv)), dim3(kBlock), 0, st, (const float4 *) pairs,
                           (const CorrHead *) d_head, thr2, d_bins);
        hipLaunchKernelGGL(k_corr_bins_sums, dim3(1), dim3(64), 0, st, (const long long *) d_bins, (int) kCorrRefitComps, d_head);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(fast_fetch(ctx, w.h_head.p, d_head, sizeof(CorrHead)));
        refined = corr_refit_from_sums(h_head->sum, h_head->poison != 0u, (double) walk.best, h_head->p0, h_head->q0, T);
        if (refined) {
            t.has = 1;
            for (int k = 0; k < 12; ++k) t.T[k] = (float) T[k];
        }
    }

    // ---- the selection with the returned transform
    unsigned char *d_labels = c.labels_out;
    int *d_idx = c.inliers_out;
    const size_t d_cap = std::min<size_t>(c.cap, mv);
    if (c.host_out) {
        if (c.labels_out) {
            WM_HIP(ctx, w.labels.reserve(m));
            d_labels = w.labels.as<unsigned char>();
        }
        WM_HIP(ctx, w.idx.reserve(d_cap * 4));
        d_idx = w.idx.as<int>();
    }
    if (d_labels) WM_HIP(ctx, hipMemsetAsync(d_labels, WM_CORR_NONE, m, st));
    hipLaunchKernelGGL(k_corr_select, dim3(blocks_of(mv)), dim3(kBlock), 0, st, (const float4 *) pairs, (const int *) pair_e, mv, t,
                       (const CorrHead *) d_head, thr2, flag, d_labels);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, flag, mv, pos));
    hipLaunchKernelGGL(k_corr_compact, dim3(blocks_of(mv)), dim3(kBlock), 0, st, (const int *) pair_e, (const unsigned *) flag,
                       (const unsigned *) pos, mv, d_idx, d_cap, d_head);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(fast_fetch(ctx, w.h_head.p, d_head, sizeof(CorrHead)));
    if (timed) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (!refined) {
        for (int k = 0; k < 12; ++k) T[k] = (double) h_head->model[k];
        T[12] = T[13] = T[14] = 0.0;
        T[15] = 1.0;
    }
    memcpy(c.T_out, T, sizeof(T));
    const size_t kept = h_head->n_out;
    *c.n_out = kept;
    if (c.stats) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b) != hipSuccess) ms = 0.f;
        c.stats->kernel_ms = ms;
        c.stats->n_inliers_model = (size_t) walk.best;
        c.stats->n_inliers = kept;
        c.stats->refined = refined ? 1 : 0;
        memcpy(c.stats->model, h_head->model, sizeof(c.stats->model));
    }
    if (c.host_out) {
        const size_t k = std::min(kept, c.cap);
        if (k) WM_HIP(ctx, hipMemcpy(c.inliers_out, d_idx, k * 4, hipMemcpyDeviceToHost));
        if (c.labels_out) WM_HIP(ctx, hipMemcpy(c.labels_out, d_labels, m, hipMemcpyDeviceToHost));
    }
    return kept > c.cap ? WM_ERR_ARG : WM_OK;
}

// Host memory: are there three valid entries at all?  (stops at the third)
bool corr_host_has_three(const CorrCall &c) {
    int found = 0;
    for (size_t e = 0; e < c.m && found < 3; ++e) {
        const long long si = c.qidx ? (long long) c.qidx[e] : (long long) e, ti = c.midx[e];
        if (si < 0 || si >= (long long) c.n_src || ti < 0 || ti >= (long long) c.n_tgt) continue;
        float p[3], q[3];
        memcpy(p, static_cast<const unsigned char *>(c.src) + (size_t) si * c.stride, sizeof(p));
        memcpy(q, static_cast<const unsigned char *>(c.tgt) + (size_t) ti * c.stride, sizeof(q));
        if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(q[0]) && std::isfinite(q[1]) &&
            std::isfinite(q[2]))
            ++found;
    }
    return found >= 3;
}

}  // namespace

}  // namespace wm

using namespace wm;

extern "C" {

void wm_corr_ransac_default_params(wm_corr_ransac_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    // correspondence_rejection_sample_consensus.h: inlier_threshold_ (0.05), max_iterations_ (1000), refine_ (false)
    p->inlier_threshold = 0.05;
    p->max_iterations = 1000;
    p->probability = 0.99;
    p->refine_model = 0;
    p->min_sample_distance = -1.0;
    p->seed = 0;
}

int wm_corr_ransac(wm_ctx *ctx, const void *src, size_t n_src, const void *tgt, size_t n_tgt, size_t stride,
                   const int32_t *query_idx, const int32_t *match_idx, size_t m, int mem, const wm_corr_ransac_params *p,
                   double T_out[16], int32_t *inliers_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out,
                   wm_corr_ransac_stats *stats) {
    if (!ctx || !n_out || !T_out || !corr_params_ok(p) || stride < 12 || (stride & 3) ||
        !(mem == WM_MEM_HOST || mem == WM_MEM_DEVICE) || !(out_mem == WM_MEM_HOST || out_mem == WM_MEM_DEVICE) ||
        n_src > 0x7FFFFFF0u || n_tgt > 0x7FFFFFF0u || m > WM_FEATURE_MAX_ROWS || (!query_idx && m > n_src) ||
        (n_src > 0 && !src) || (n_tgt > 0 && !tgt) || (m > 0 && !match_idx) || (cap > 0 && !inliers_out))
        return WM_ERR_ARG;
    *n_out = 0;
    if (stats) {
        *stats = wm_corr_ransac_stats{};
        stats->best_hypothesis = -1;
    }
    if (m < 3 || n_src == 0 || n_tgt == 0) return WM_NOT_CONVERGED;  // (no sample: no device is touched)
    const CorrCall c{src, n_src, tgt, n_tgt, stride, query_idx, match_idx, m, mem, p, T_out, inliers_out, cap,
                     out_mem == WM_MEM_HOST, n_out, labels_out, stats};
    if (mem == WM_MEM_HOST && !corr_host_has_three(c)) return WM_NOT_CONVERGED;  // (the same, seen on the host)
    return corr_call(ctx, c);
}

int wm_corr_hypothesis(const float p[9], const float q[9], float min_d2, float T_out[12]) {
    if (!p || !q || !T_out) return WM_ERR_ARG;
    return corr_hypothesis(p, q, min_d2, T_out) == kCorrValid ? 1 : 0;
}

int wm_debug_corr_hypotheses(wm_ctx *ctx, uint64_t j0, int count, float *T_out, uint32_t *flags_out) {
    if (!ctx || count < 1 || count > kCorrMaxRound || !T_out || !flags_out) return WM_ERR_ARG;
    CorrWs *w = static_cast<CorrWs *>(ctx->corr);
    if (!w || !w->have || w->mv < 3) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_HIP(ctx, w->round.reserve(corr_round_bytes(kCorrMaxRound)));
    unsigned *d_words = w->round.as<unsigned>();
    float4 *d_T3 = reinterpret_cast<float4 *>(d_words + corr_T3_at(kCorrMaxRound));
    hipLaunchKernelGGL(k_corr_hypotheses, dim3(blocks_of((size_t) count)), dim3(kBlock), 0, ctx->stream,
                       (const float4 *) w->pairs.as<float4>(), w->mv, w->seed, (unsigned long long) j0, (unsigned) count,
                       w->min_d2, d_T3, d_words, (unsigned *) nullptr);
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    WM_HIP(ctx, hipMemcpy(T_out, d_T3, (size_t) count * 12 * sizeof(float), hipMemcpyDeviceToHost));
    WM_HIP(ctx, hipMemcpy(flags_out, d_words, (size_t) count * 4, hipMemcpyDeviceToHost));
    return WM_OK;
}

}  // extern "C"
