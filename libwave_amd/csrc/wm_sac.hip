// wm_sac.hip -- plane segmentation on the device: pcl::SACSegmentation with a plane model and SAC_RANSAC as one cloud-in /
// plane-out call (wm_sac_segment), shaped like wm_cluster_extract: the call packs the cloud and works in a workspace of
// its own on the context; and the same for a queue of scans in one call (wm_sac_segment_batch).  No grid, no
// neighbour search: the hot loop is hypotheses x points plane tests.
//
// The rule is stated in include/wavematch.h (written from PCL 1.8 ransac.hpp, sac_model_plane.hpp and
// sac_segmentation.hpp; PCL is not linked, the checker is tests/sac_reference.py).  The hypothesis stream is a function
// of (seed, j, n), so the device evaluates it in ROUNDS of up to `sac_round` entries and the host walks each round's
// (flag, count) pairs in stream order with PCL's loop (wm_sac_walk.hpp); entries behind the stopping point are
// discarded.  A round never holds more entries than the loop can still count as iterations (max_iterations + 1 - it):
// only skipped entries make another round necessary.  How the stream is cut into rounds changes no output.
//
// Launches of a single call: pack, then per round
//   k_sac_hypotheses   one lane per stream entry: indices -> three point loads -> plane -> validity; a float4 and a flag
//   k_sac_count        the hot kernel: a lane keeps kSacPts points in registers and loops over the round's planes, read
//                      through a wave-uniform index (scalar loads); per plane a ballot and a popcount per point slot,
//                      accumulated per workgroup in LDS; one integer atomicAdd per plane and workgroup at its end.
//                      Integer counts: order-independent.  The points are read once per round.
//   one fetch of the round (planes, flags, counts)
// and behind the loop k_sac_sums (the refit's nine sums of the model's inliers as exact integer limbs, wm_bins.hpp's
// splitting with a bins array of this call's own) + one fetch of the limbs, the 3 x 3 eigenproblem on the host, then
// k_sac_select (flags and labels) -> exclusive_scan -> k_sac_compact and one fetch of the count.
//
// A batch (sac_batch below) runs the same device functions with a scan dimension: wm_scan_table.hpp's table and pack,
// per round a small table of the LIVE scans (each with its own j0 and R), one hypotheses launch over all entries of the
// round, one count launch whose workgroups are bound to ONE scan each, one fetch of the (flag, count) pairs; behind the
// rounds the models are recomputed from their stream entries, the refit's bins are summed on the device in the single
// call's order, and one select / scan / compact covers the batch.
#include <float.h>
#include <string.h>

#include "wm_bins.hpp"
#include "wm_sac_walk.hpp"
#include "wm_scan_table.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace wm {

namespace {

constexpr int kSacMaxRound = 1024;            // the option's upper end: s_cnt of the count kernels
constexpr int kSacPts = 4;                    // points a lane of the count kernels keeps in registers
constexpr int kSacTile = kBlock * kSacPts;    // points of a workgroup's tile
constexpr unsigned kSacMaxBlocks = 2048;      // count workgroups of a cloud at the most (8 per CU): each walks tiles
// the refit's bins: kSacBins bins x kBinLimbs limb rows x kSacStride words; components 0 ... 8 in use ([0..2] sum dx dy
// dz, [3..8] sum dxdx dxdy dxdz dydy dydz dzdz), word kSacPoison of limb row 0 counts sums the limbs cannot hold.
// A limb of one addend is below 2^40 and a bin's word holds 2^63: 2^23 points per bin, 2^31 points over 256 bins.
constexpr int kSacBins = 256;
constexpr int kSacStride = 16;
constexpr int kSacPoison = kSacStride - 1;
constexpr int kSacBinSize = kBinLimbs * kSacStride;  // words of a bin
constexpr size_t kSacBinWords = (size_t) kSacBins * kSacBinSize;

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

// ------------------------------------------------------------------ the steps both entry points run (device)
// Entry j of the stream of a cloud of n points: its plane and its flag (a skipped entry's plane is zero).  Every
// operation is rounded and sqrt and the division are the correctly rounded ones, so the plane is a function of the
// entry -- wherever it is evaluated (a round's lane; the lane that recomputes a batch's models).
__device__ __forceinline__ unsigned sac_hypothesis(const float4 *__restrict__ pts, unsigned n, unsigned long long seed,
                                                   unsigned long long j, const SacAxis &ax, float4 &pl) {
    unsigned i[3];
    sac_sample(seed, j, n, i);  // (each index < n by construction)
    const float4 p0 = pts[i[0]], p1 = pts[i[1]], p2 = pts[i[2]];
    const float ux = __fsub_rn(p1.x, p0.x), uy = __fsub_rn(p1.y, p0.y), uz = __fsub_rn(p1.z, p0.z);
    const float vx = __fsub_rn(p2.x, p0.x), vy = __fsub_rn(p2.y, p0.y), vz = __fsub_rn(p2.z, p0.z);
    const float cx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
    const float cy = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
    const float cz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(cx, cx), __fmul_rn(cy, cy)), __fmul_rn(cz, cz));
    unsigned flag = kSacSkipped;
    pl = make_float4(0.f, 0.f, 0.f, 0.f);
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
    return flag;
}

// The count of ONE cloud's points against R planes by workgroup `wb` of the `nb` that share the cloud.  The workgroup
// walks tiles of kSacTile points; of a tile a lane holds kSacPts points (slot u: point tile * kSacTile + u * kBlock +
// thread, coalesced) and tests them against every valid plane.  planes and flags are read at a wave-uniform index.  A
// point behind the cloud's end and a non-finite point (NaN since the pack) fail dist < thr.  finite_out != nullptr: the
// cloud's finite points are counted on the way.
__device__ __forceinline__ void sac_count_tiles(const float4 *__restrict__ pts, unsigned n, const float4 *__restrict__ planes,
                                                const unsigned *__restrict__ flags, unsigned R, float thr,
                                                unsigned *__restrict__ counts, unsigned wb, unsigned nb,
                                                unsigned *__restrict__ finite_out) {
    __shared__ unsigned s_cnt[kSacMaxRound];
    for (unsigned j = threadIdx.x; j < R; j += kBlock) s_cnt[j] = 0u;
    __syncthreads();
    const bool lane0 = (threadIdx.x & 63u) == 0u;
    const float nanv = __builtin_nanf("");
    unsigned nfin = 0u;
    for (size_t t0 = (size_t) wb * kSacTile; t0 < n; t0 += (size_t) nb * kSacTile) {
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

// A wave's share of the refit's sums: the nine terms of its lanes' inliers (in: the lane's point is one), relative to
// p0, into bin b.  A point's nine terms are doubles formed from exact differences, each split into limbs (bins_split: a
// function of the term alone); the limbs are integers, so the wave's shuffles and the bin's atomics add them exactly in
// any order.  Called by every lane of the wave.
__device__ __forceinline__ void sac_sums_wave(bool in, const float4 &p, const float4 &p0, long long *__restrict__ b) {
    if (__ballot(in) == 0ull) return;  // (the whole wave)
    const double dx = in ? (double) p.x - (double) p0.x : 0.0, dy = in ? (double) p.y - (double) p0.y : 0.0,
                 dz = in ? (double) p.z - (double) p0.z : 0.0;
    const double term[kSacComps] = {dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
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

// Component c of a cloud's sums from its first `nbins` bins: the bins' values (bins_value: the same double on the host
// and on the device) added in DOUBLE, bin 0 first, every add rounded.  The refit's bits depend on which wave fed which
// bin and on this order, so both entry points sum here.  A bin that no wave fed is +0.0 and changes no sum: a cloud of
// fewer than kSacBins waves needs only its waves' bins.
__device__ __host__ inline double sac_bins_sum(const long long *bins, unsigned nbins, int c) {
    double s = 0.0;
    for (unsigned b = 0; b < nbins; ++b) {  // (a bin's limbs are exact integers: its value is a function of the inliers)
        const long long *w = bins + (size_t) b * kSacBinSize + c;
        s += bins_value(w[0], w[kSacStride], w[2 * kSacStride]);
    }
    return s;
}

// ------------------------------------------------------------------ the single call's kernels
// One lane per entry j0 + e of the round.  counts[e] = 0 for the count kernel behind it.
__global__ void __launch_bounds__(kBlock)
    k_sac_hypotheses(const float4 *__restrict__ pts, unsigned n, unsigned long long seed, unsigned long long j0, unsigned R,
                     SacAxis ax, float4 *__restrict__ planes, unsigned *__restrict__ flags, unsigned *__restrict__ counts) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= R) return;
    float4 pl;
    const unsigned flag = sac_hypothesis(pts, n, seed, j0 + e, ax, pl);
    planes[e] = pl;
    flags[e] = flag;
    counts[e] = 0u;
}

// The hot kernel (sac_count_tiles): the grid's workgroups share the cloud.  finite_out: the first round's.
__global__ void __launch_bounds__(kBlock)
    k_sac_count(const float4 *__restrict__ pts, unsigned n, const float4 *__restrict__ planes,
                const unsigned *__restrict__ flags, unsigned R, float thr, unsigned *__restrict__ counts,
                unsigned *__restrict__ finite_out) {
    sac_count_tiles(pts, n, planes, flags, R, thr, counts, blockIdx.x, gridDim.x, finite_out);
}

// The refit's sums over the MODEL's inliers, relative to p0 = pts[i0] (the winning sample's first point, finite since
// its entry was valid); bin = the wave's number mod kSacBins.  tail: the words behind the bins, where p0 goes for the host.
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
    const unsigned wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    sac_sums_wave(in, p, p0, bins + (size_t) (wave % kSacBins) * kSacBinSize);
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

// ------------------------------------------------------------------ a batch's kernels
struct SacRow {  // a live scan in a round
    unsigned long long j0;  // its first stream entry of the round
    unsigned scan, R;       // the scan; its entries of the round (>= 1)
    unsigned e0, cb0;       // the first entry's place in the round's arrays; its first count workgroup
    unsigned off, n;        // the scan's first batch position; its points
    unsigned nb, pad;       // its count workgroups (>= 1)
};

struct SacFin {  // a scan behind the rounds
    long long best_j;       // its model's stream entry, -1: no model
    unsigned refit, bin0;   // whether its sums are formed; its first bin
    unsigned nbins, has;    // min(kSacBins, its waves); whether `coef` holds its returned plane (the selection)
    unsigned pad[2];
    float4 coef;
};

struct SacOut {  // what the host needs of a scan behind the rounds
    double sum[kSacComps];
    float4 model, p0;
    unsigned poison, pad[3];
};

// One lane per entry of the round, over all live scans.
__global__ void __launch_bounds__(kBlock)
    k_sac_hypotheses_batch(const float4 *__restrict__ pts, const SacRow *__restrict__ rows, unsigned L, unsigned E,
                           unsigned long long seed, SacAxis ax, float4 *__restrict__ planes, unsigned *__restrict__ flags,
                           unsigned *__restrict__ counts) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const SacRow me = rows[cl_find(rows, L, e, [](const SacRow &r) { return r.e0; })];
    float4 pl;
    const unsigned flag = sac_hypothesis(pts + me.off, me.n, seed, me.j0 + (e - me.e0), ax, pl);
    planes[e] = pl;
    flags[e] = flag;
    counts[e] = 0u;
}

// A workgroup is bound to tiles of ONE scan: the LDS counters and the one atomic per plane and workgroup are the scan's.
__global__ void __launch_bounds__(kBlock)
    k_sac_count_batch(const float4 *__restrict__ pts, const SacRow *__restrict__ rows, unsigned L,
                      const float4 *__restrict__ planes, const unsigned *__restrict__ flags, float thr,
                      unsigned *__restrict__ counts) {
    const SacRow me = rows[cl_find(rows, L, blockIdx.x, [](const SacRow &r) { return r.cb0; })];
    sac_count_tiles(pts + me.off, me.n, planes + me.e0, flags + me.e0, me.R, thr, counts + me.e0, blockIdx.x - me.cb0, me.nb,
                    nullptr);
}

// One lane per scan: the model is entry best_j of the scan's stream, evaluated again, and p0 its sample's first point.
__global__ void __launch_bounds__(kBlock)
    k_sac_models(const ClScan *__restrict__ tab, const SacFin *__restrict__ fin, unsigned S, const float4 *__restrict__ pts,
                 unsigned long long seed, SacAxis ax, SacOut *__restrict__ out) {
    const unsigned k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= S) return;
    float4 pl = make_float4(0.f, 0.f, 0.f, 0.f), p0 = pl;
    const long long bj = fin[k].best_j;
    if (bj >= 0) {
        const ClScan me = tab[k];
        (void) sac_hypothesis(pts + me.off, me.n, seed, (unsigned long long) bj, ax, pl);
        unsigned i[3];
        sac_sample(seed, (unsigned long long) bj, me.n, i);
        p0 = pts[me.off + i[0]];
    }
    out[k].model = pl;
    out[k].p0 = p0;
    out[k].poison = 0u;
}

// k_sac_sums over batch positions.  The workgroups are aligned to each scan's start (blk0), so a wave's number INSIDE
// its scan mod kSacBins is its bin, exactly as in the single call; the scan's bins start at bin0.
__global__ void __launch_bounds__(kBlock)
    k_sac_sums_batch(const ClScan *__restrict__ tab, unsigned S, const SacFin *__restrict__ fin, const SacOut *__restrict__ out,
                     const float4 *__restrict__ pts, float thr, long long *__restrict__ bins) {
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const SacFin f = fin[k];
    if (!f.refit) return;  // (the whole workgroup)
    const ClScan me = tab[k];
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    const float4 pl = out[k].model, p0 = out[k].p0;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool in = false;
    if (i < me.n) {
        p = pts[me.off + i];
        in = sac_dist(pl, p.x, p.y, p.z) < thr;
    }
    const unsigned wave = (blockIdx.x - me.blk0) * (kBlock / 64) + (threadIdx.x >> 6);
    sac_sums_wave(in, p, p0, bins + ((size_t) f.bin0 + wave % kSacBins) * kSacBinSize);
}

// A wave per scan: its bins into the nine doubles (lane c: component c, sac_bins_sum) and the poison flag.
__global__ void __launch_bounds__(64)
    k_sac_bins_sums(const SacFin *__restrict__ fin, const long long *__restrict__ bins, SacOut *__restrict__ out) {
    const unsigned k = blockIdx.x;
    const SacFin f = fin[k];
    if (!f.refit) return;
    const long long *b = bins + (size_t) f.bin0 * kSacBinSize;
    if (threadIdx.x < (unsigned) kSacComps) out[k].sum[threadIdx.x] = sac_bins_sum(b, f.nbins, (int) threadIdx.x);
    bool poison = false;
    for (unsigned j = threadIdx.x; j < f.nbins; j += 64u) poison = poison || b[(size_t) j * kSacBinSize + kSacPoison] != 0ll;
    const bool any = __ballot(poison) != 0ull;
    if (threadIdx.x == 0u) out[k].poison = any ? 1u : 0u;
}

// k_sac_select over batch positions with the scans' returned planes.  flag: inlier, or with `negative` finite
// non-inlier; a scan without a model keeps nothing and its labels are NONE.  labels: the scans' n entries one after the
// other (aux0: the scan's first label).  ninl != nullptr: the scans' inliers are counted (integers).
__global__ void __launch_bounds__(kBlock)
    k_sac_select_batch(const ClScan *__restrict__ tab, unsigned S, const SacFin *__restrict__ fin, const float4 *__restrict__ pts,
                       float thr, int negative, unsigned *__restrict__ flag, unsigned char *__restrict__ labels,
                       unsigned *__restrict__ ninl) {
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    const bool has = fin[k].has != 0u;
    bool in = false, finite = false;
    if (i < me.n) {
        const float4 pl = fin[k].coef;
        const float4 p = pts[me.off + i];
        finite = p.x == p.x;
        in = has && sac_dist(pl, p.x, p.y, p.z) < thr;
        flag[me.off + i] = (negative ? has && finite && !in : in) ? 1u : 0u;
        if (labels)
            labels[(size_t) me.aux0 + i] =
                (unsigned char) (!has ? WM_SAC_NONE : in ? WM_SAC_INLIER : finite ? WM_SAC_OUTLIER : WM_SAC_NONE);
    }
    if (ninl) {
        const unsigned c = (unsigned) __popcll(__ballot(in));
        if ((threadIdx.x & 63u) == 0u && c) atomicAdd(&ninl[k], c);
    }
}

// pos = the exclusive scan of flag over the batch (total + 1 entries).  The first `blocks` workgroups write the kept
// entries: the index INSIDE the scan and, where wanted, the point's record; the grid's first S + 1 threads write the
// scans' offsets.
__global__ void __launch_bounds__(kBlock)
    k_sac_compact_batch(const ClScan *__restrict__ tab, unsigned S, unsigned blocks, unsigned total,
                        const float4 *__restrict__ pts, const unsigned *__restrict__ flag, const unsigned *__restrict__ pos,
                        int *__restrict__ idx_out, size_t cap, unsigned char *__restrict__ pout, size_t out_stride,
                        unsigned *__restrict__ offs) {
    const size_t g = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (g <= S) offs[g] = pos[g < S ? tab[g].off : total];
    if (blockIdx.x >= blocks) return;
    const unsigned k = cl_by_block(tab, S, blockIdx.x);
    const ClScan me = tab[k];
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    if (i >= me.n || !flag[me.off + i]) return;
    const unsigned at = pos[me.off + i];
    if (at >= cap) return;
    idx_out[at] = (int) i;
    if (pout) cl_write_record(pout, at, out_stride, pts[me.off + i]);
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

}  // namespace

// The context's workspace of the plane segmentation: its own buffers, shared with nothing else on the context.
struct SacWs {
    DevBuf pts;            // the packed cloud; a batch: the packed clouds, batch positions
    DevBuf round;          // a round: [R float4 planes][R flags][R counts][4 words: the finite points, the inliers]
                           // a batch: [7 S words: the pack's boxes and finite counts][E flags][E counts] ... [E planes]
    DevBuf bins;           // the refit's limbs + the tail (p0); a batch: the scans' bins
    DevBuf flag, pos;      // the selection's scan
    DevBuf idx, labels;    // host outputs on their way
    DevBuf pout;           // a batch: the points of a caller in host memory on their way
    DevBuf rows, fin, out, offs;  // a batch: the round's table, the scans' SacFin and SacOut, the offsets and inlier counts
    PairStage stage;       // a batch's scan table and host clouds up (wm_stage.hpp)
    PinnedBuf h_round, h_bins;
    PinnedBuf h_rows, h_fin, h_out;
};

void sac_release(wm_ctx *ctx) {
    SacWs *w = static_cast<SacWs *>(ctx->sac);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts, &w->round, &w->bins, &w->flag, &w->pos, &w->idx, &w->labels, &w->pout, &w->rows, &w->fin,
                      &w->out, &w->offs};
    for (DevBuf *b : bufs) b->release();
    w->stage.release();
    PinnedBuf *pins[] = {&w->h_round, &w->h_bins, &w->h_rows, &w->h_fin, &w->h_out};
    for (PinnedBuf *b : pins) b->release();
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

SacAxis sac_axis(const wm_sac_params *p) {
    SacAxis ax{p->model, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p->model != WM_SAC_PLANE) {
        const double l = std::sqrt((p->axis[0] * p->axis[0] + p->axis[1] * p->axis[1]) + p->axis[2] * p->axis[2]);
        ax.x = (float) (p->axis[0] / l);
        ax.y = (float) (p->axis[1] / l);
        ax.z = (float) (p->axis[2] / l);
        ax.cos_eps = (float) std::cos(p->eps_angle);
        ax.sin_eps = (float) std::sin(p->eps_angle);
    }
    return ax;
}

unsigned sac_round_max(const wm_ctx *ctx) { return (unsigned) std::min(std::max(ctx->tune_sac_round, 1), kSacMaxRound); }

unsigned sac_count_blocks(size_t n) { return (unsigned) std::min<size_t>((n + kSacTile - 1) / kSacTile, kSacMaxBlocks); }

// The single call's refit: the sums from its kSacBins bins (fetched), then the plane of the sums (wm_sac_walk.hpp).
bool sac_refit(const long long *bins, const float *p0, double m, const float model[4], float out[4]) {
    double sum[kSacComps];
    for (int c = 0; c < kSacComps; ++c) sum[c] = sac_bins_sum(bins, kSacBins, c);
    bool poison = false;
    for (int b = 0; b < kSacBins; ++b) poison = poison || bins[(size_t) b * kSacBinSize + kSacPoison] != 0ll;
    return sac_plane_from_sums(sum, poison, p0, m, model, out);
}

int sac_run(wm_ctx *ctx, const void *pts_in, size_t n, size_t stride, int mem, const wm_sac_params *p, float *coef_out,
            int32_t *indices_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out, wm_sac_stats *stats) {
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->sac) ctx->sac = new SacWs();
    SacWs &w = *static_cast<SacWs *>(ctx->sac);
    hipStream_t st = ctx->stream;
    const bool host_out = out_mem == WM_MEM_HOST, timed = stats != nullptr;
    const unsigned nu = (unsigned) n;
    const unsigned Rmax = sac_round_max(ctx);
    const float thr = sac_threshold(p->distance_threshold);
    const SacAxis ax = sac_axis(p);

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
    const unsigned count_blocks = sac_count_blocks(n);

    // ---- PCL's loop over the stream, a round at a time (wm_sac_walk.hpp)
    SacWalk walk;
    walk.start(p->max_iterations, p->probability, n);
    float model[4] = {0.f, 0.f, 0.f, 0.f};
    size_t n_finite = 0;
    while (walk.going) {
        const unsigned R = walk.round_size(Rmax);
        hipLaunchKernelGGL(k_sac_hypotheses, dim3(blocks_of(R)), dim3(kBlock), 0, st, (const float4 *) d_pts, nu,
                           (unsigned long long) p->seed, walk.j, R, ax, d_planes, d_flags, d_counts);
        hipLaunchKernelGGL(k_sac_count, dim3(count_blocks), dim3(kBlock), 0, st, (const float4 *) d_pts, nu,
                           (const float4 *) d_planes, (const unsigned *) d_flags, R, thr, d_counts,
                           walk.rounds == 0 ? d_res : (unsigned *) nullptr);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(fast_fetch(ctx, w.h_round.p, w.round.p, round_bytes));
        if (walk.rounds == 0) n_finite = h_res[0];
        walk.feed_round(h_flags, h_counts, R, [&](unsigned e) { memcpy(model, &h_planes[e], sizeof(model)); });
    }
    const long long best = walk.best, best_j = walk.best_j;
    if (stats) {
        stats->n_finite = n_finite;
        stats->iterations = (int) walk.it;
        stats->skipped = (int) walk.skipped;
        stats->rounds = walk.rounds;
        stats->hypotheses = (long long) walk.j;
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

// ------------------------------------------------------------------ a batch
// A fetch of a batch: small ones by fast_fetch's one workgroup, large ones (a long round of many scans) by the copy engine.
int sac_fetch(wm_ctx *ctx, void *dst_pinned, const void *src_dev, size_t bytes) {
    if (bytes <= ((size_t) 64 << 10)) return fast_fetch(ctx, dst_pinned, src_dev, bytes);
    WM_HIP(ctx, hipMemcpyAsync(dst_pinned, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

struct SacBatchCall {
    const wm_sac_scan *scans;
    unsigned S;
    size_t stride;
    int mem;
    const wm_sac_params *p;
    int negative;
    float *coefficients_out;
    int32_t *indices_out;
    size_t cap;
    void *points_out;
    size_t out_stride;
    bool host_out;
    size_t *offsets_out;
    uint8_t *labels_out;
    int *status;
    wm_sac_stats *stats;
    float *kernel_ms;
};

// The batch (arguments checked, the outputs' defaults written, at least one scan of n >= 3).  Launches and host waits:
// the front (upload, pack), per round of the longest-living scan the round's table up, two launches and one fetch, then
// the models (and the refit's sums) with one fetch, the coefficients up, select / scan / compact and one fetch of the
// offsets -- whatever the number of scans.
int sac_batch(wm_ctx *ctx, const SacBatchCall &c) {
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->sac) ctx->sac = new SacWs();
    SacWs &w = *static_cast<SacWs *>(ctx->sac);
    hipStream_t st = ctx->stream;
    const wm_sac_params *p = c.p;
    const unsigned S = c.S;
    const unsigned Rmax = sac_round_max(ctx);
    const float thr = sac_threshold(p->distance_threshold);
    const SacAxis ax = sac_axis(p);
    const unsigned long long seed = (unsigned long long) p->seed;

    // ---- the front.  A scan of n < 3 has no sample: it gets no batch position and no workgroup (n = 0 in the table);
    // aux0 is a scan's first label, which counts such a scan's points
    std::vector<wm_sac_scan> rows_in(c.scans, c.scans + S);
    std::vector<SacWalk> walk(S);
    std::vector<unsigned> live;
    size_t label_total = 0, E0 = 0;
    bool tiny = false;
    for (unsigned k = 0; k < S; ++k) {
        label_total += c.scans[k].n;
        if (c.scans[k].n < 3) {
            tiny = tiny || c.scans[k].n > 0;
            rows_in[k].n = 0;
            continue;
        }
        walk[k].start(p->max_iterations, p->probability, c.scans[k].n);
        live.push_back(k);
        E0 += walk[k].round_size(Rmax);  // (the first round is the largest: R never grows and no scan comes back)
    }
    // the round's words: [6 S boxes][S finite counts][E flags][E counts], the planes behind them at a fixed place
    const size_t planes_at = (7 * (size_t) S + 2 * E0 + 3) & ~(size_t) 3;  // (words; a float4's alignment)
    const size_t round_bytes = planes_at * 4 + E0 * sizeof(float4);
    WM_HIP(ctx, w.h_round.reserve(std::max((size_t) S + 2 * E0, 2 * (size_t) S + 1) * 4));  // (a round; the offsets' fetch)
    WM_HIP(ctx, w.rows.reserve((live.size() + 1) * sizeof(SacRow)));
    WM_HIP(ctx, w.h_rows.reserve((live.size() + 1) * sizeof(SacRow)));
    WM_HIP(ctx, w.fin.reserve((size_t) S * sizeof(SacFin)));
    WM_HIP(ctx, w.h_fin.reserve((size_t) S * sizeof(SacFin)));
    WM_HIP(ctx, w.out.reserve((size_t) S * sizeof(SacOut)));
    WM_HIP(ctx, w.h_out.reserve((size_t) S * sizeof(SacOut)));
    WM_HIP(ctx, w.offs.reserve((2 * (size_t) S + 1) * 4));
    ScanTable T;
    WM_TRY(scan_table_pack(ctx, w.stage, rows_in.data(), S, c.stride, c.mem, w.pts, w.round, round_bytes, &T));
    const size_t total = T.total;
    {  // the labels' places; the table goes up again with them (the pack did not read them)
        size_t at = 0;
        for (unsigned k = 0; k < S; ++k) {
            T.tab[k].aux0 = (unsigned) at;
            at += c.scans[k].n;
        }
        WM_HIP(ctx, hipMemcpyAsync(w.stage.up.dev.p, w.stage.up.host.p, T.table_bytes, hipMemcpyHostToDevice, st));
    }
    const float4 *d_pts = w.pts.as<float4>();
    unsigned *d_words = w.round.as<unsigned>();
    float4 *d_planes = reinterpret_cast<float4 *>(d_words + planes_at);
    const unsigned *h_words = w.h_round.as<unsigned>();
    SacRow *h_rows = w.h_rows.as<SacRow>();

    // ---- the rounds: every live scan walks its own stream, R_k = min(sac_round, max_iterations + 1 - it_k) entries
    for (int round = 0; !live.empty(); ++round) {
        unsigned E = 0, cb = 0;
        const unsigned L = (unsigned) live.size();
        for (unsigned r = 0; r < L; ++r) {
            const unsigned k = live[r];
            SacRow &row = h_rows[r];
            row.j0 = walk[k].j;
            row.scan = k;
            row.R = walk[k].round_size(Rmax);
            row.e0 = E;
            row.cb0 = cb;
            row.off = T.tab[k].off;
            row.n = T.tab[k].n;
            row.nb = sac_count_blocks(row.n);
            row.pad = 0;
            E += row.R;
            cb += row.nb;
        }
        h_rows[L] = SacRow{0ull, S, 0u, E, cb, 0u, 0u, 0u, 0u};
        unsigned *d_flags = d_words + 7 * (size_t) S, *d_counts = d_flags + E;
        WM_HIP(ctx, hipMemcpyAsync(w.rows.p, h_rows, ((size_t) L + 1) * sizeof(SacRow), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_sac_hypotheses_batch, dim3(blocks_of(E)), dim3(kBlock), 0, st, d_pts,
                           (const SacRow *) w.rows.as<SacRow>(), L, E, seed, ax, d_planes, d_flags, d_counts);
        hipLaunchKernelGGL(k_sac_count_batch, dim3(cb), dim3(kBlock), 0, st, d_pts, (const SacRow *) w.rows.as<SacRow>(), L,
                           (const float4 *) d_planes, (const unsigned *) d_flags, thr, d_counts);
        WM_HIP(ctx, hipGetLastError());
        // the round's (flag, count) pairs of the live scans; in front of the first round's the pack's finite counts
        const unsigned *h_flags = h_words + S;
        if (round == 0) {
            WM_TRY(sac_fetch(ctx, w.h_round.p, d_words + 6 * (size_t) S, ((size_t) S + 2 * (size_t) E) * 4));
            if (c.stats)
                for (unsigned k : live) c.stats[k].n_finite = h_words[k];
        } else {
            WM_TRY(sac_fetch(ctx, w.h_round.as<unsigned>() + S, d_flags, 2 * (size_t) E * 4));
        }
        const unsigned *h_counts = h_flags + E;
        std::vector<unsigned> next;
        for (unsigned r = 0; r < L; ++r) {
            const unsigned k = live[r];
            walk[k].feed_round(h_flags + h_rows[r].e0, h_counts + h_rows[r].e0, h_rows[r].R);
            if (walk[k].going) next.push_back(k);  // a scan that has stopped is not read again
        }
        live.swap(next);
    }

    // ---- behind the rounds: the loop's counters; which scans have a model, which are refitted, their bins
    SacFin *h_fin = w.h_fin.as<SacFin>();
    size_t n_bins = 0;
    bool any_model = false;
    for (unsigned k = 0; k < S; ++k) {
        const SacWalk &wk = walk[k];
        SacFin &f = h_fin[k];
        f = SacFin{};
        f.best_j = -1;
        if (c.scans[k].n < 3) continue;
        if (c.stats) {
            wm_sac_stats &s = c.stats[k];
            s.iterations = (int) wk.it;
            s.skipped = (int) wk.skipped;
            s.rounds = wk.rounds;
            s.hypotheses = (long long) wk.j;
            s.best_hypothesis = wk.best_j;
        }
        if (wk.best_j < 0) continue;
        any_model = true;
        f.best_j = wk.best_j;
        if (p->optimize_coefficients && wk.best >= 4) {
            const size_t waves = ((size_t) T.tab[k].n + 63) / 64;
            f.refit = 1u;
            f.bin0 = (unsigned) n_bins;
            f.nbins = (unsigned) std::min<size_t>(kSacBins, waves);
            n_bins += f.nbins;
        }
    }
    // the outputs' places: the caller's own in device memory, else the workspace's
    unsigned char *d_labels = c.labels_out;
    if (c.labels_out && c.host_out) {
        WM_HIP(ctx, w.labels.reserve(label_total));
        d_labels = w.labels.as<unsigned char>();
    }
    auto finish = [&](float *ms) -> int {  // (the stream has been waited for; ev_b lies behind the last launch)
        if (hipEventElapsedTime(ms, ctx->ev_a, ctx->ev_b) != hipSuccess) *ms = 0.f;
        if (c.kernel_ms) *c.kernel_ms = *ms;
        if (c.stats)
            for (unsigned k = 0; k < S; ++k)
                if (c.scans[k].n >= 3) c.stats[k].kernel_ms = *ms;
        if (c.host_out && c.labels_out) WM_HIP(ctx, hipMemcpy(c.labels_out, d_labels, label_total, hipMemcpyDeviceToHost));
        return WM_OK;
    };
    float ms = 0.f;
    if (!any_model) {  // every slice is empty and every label NONE
        if (d_labels) WM_HIP(ctx, hipMemsetAsync(d_labels, 0, label_total, st));
        WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
        WM_HIP(ctx, hipStreamSynchronize(st));
        return finish(&ms);
    }

    // ---- the models again from their entries, the refit's sums in the single call's bins and order; one fetch
    const ClScan *d_tab = T.d_tab;
    const SacFin *d_fin = w.fin.as<SacFin>();
    SacOut *d_out = w.out.as<SacOut>();
    WM_HIP(ctx, hipMemcpyAsync(w.fin.p, h_fin, (size_t) S * sizeof(SacFin), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sac_models, dim3(blocks_of(S)), dim3(kBlock), 0, st, d_tab, d_fin, S, d_pts, seed, ax, d_out);
    if (n_bins) {
        WM_HIP(ctx, w.bins.reserve(n_bins * kSacBinSize * sizeof(long long)));
        long long *d_bins = w.bins.as<long long>();
        WM_HIP(ctx, hipMemsetAsync(d_bins, 0, n_bins * kSacBinSize * sizeof(long long), st));
        hipLaunchKernelGGL(k_sac_sums_batch, dim3((unsigned) T.blocks), dim3(kBlock), 0, st, d_tab, S, d_fin,
                           (const SacOut *) d_out, d_pts, thr, d_bins);
        hipLaunchKernelGGL(k_sac_bins_sums, dim3(S), dim3(64), 0, st, d_fin, (const long long *) d_bins, d_out);
    }
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(sac_fetch(ctx, w.h_out.p, d_out, (size_t) S * sizeof(SacOut)));
    const SacOut *h_out = w.h_out.as<SacOut>();
    std::vector<int> refined(S, 0);
    for (unsigned k = 0; k < S; ++k) {
        SacFin &f = h_fin[k];
        if (f.best_j < 0) continue;
        const SacOut &o = h_out[k];
        const float model[4] = {o.model.x, o.model.y, o.model.z, o.model.w};
        const float p0[3] = {o.p0.x, o.p0.y, o.p0.z};
        float coef[4] = {model[0], model[1], model[2], model[3]};
        if (f.refit) {
            if (sac_plane_from_sums(o.sum, o.poison != 0u, p0, (double) walk[k].best, model, coef)) refined[k] = 1;
            else memcpy(coef, model, sizeof(coef));
        }
        f.has = 1u;
        f.coef = make_float4(coef[0], coef[1], coef[2], coef[3]);
        memcpy(c.coefficients_out + 4 * (size_t) k, coef, sizeof(coef));
        c.status[k] = WM_OK;
        if (c.stats) {
            c.stats[k].n_inliers_model = (size_t) walk[k].best;
            memcpy(c.stats[k].model_coefficients, model, sizeof(model));
            c.stats[k].refined = refined[k];
        }
    }

    // ---- the selection with the returned coefficients, over the batch
    WM_HIP(ctx, w.flag.reserve(total * 4));
    WM_HIP(ctx, w.pos.reserve((total + 1) * 4));
    const size_t d_cap = std::min(c.cap, total);
    int *d_idx = c.indices_out;
    unsigned char *d_pout = static_cast<unsigned char *>(c.points_out);
    if (c.host_out) {
        WM_HIP(ctx, w.idx.reserve(d_cap * 4));
        d_idx = w.idx.as<int>();
        if (c.points_out) {
            WM_HIP(ctx, w.pout.reserve(d_cap * c.out_stride));
            d_pout = w.pout.as<unsigned char>();
        }
    }
    unsigned *flag = w.flag.as<unsigned>(), *pos = w.pos.as<unsigned>();
    unsigned *d_offs = w.offs.as<unsigned>(), *d_ninl = d_offs + S + 1;
    WM_HIP(ctx, hipMemcpyAsync(w.fin.p, h_fin, (size_t) S * sizeof(SacFin), hipMemcpyHostToDevice, st));
    if (c.negative) WM_HIP(ctx, hipMemsetAsync(d_ninl, 0, (size_t) S * 4, st));
    if (d_labels && tiny) WM_HIP(ctx, hipMemsetAsync(d_labels, 0, label_total, st));  // (no workgroup writes a tiny scan's)
    hipLaunchKernelGGL(k_sac_select_batch, dim3((unsigned) T.blocks), dim3(kBlock), 0, st, d_tab, S, d_fin, d_pts, thr,
                       c.negative, flag, d_labels, c.negative ? d_ninl : (unsigned *) nullptr);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, flag, total, pos));
    hipLaunchKernelGGL(k_sac_compact_batch, dim3(std::max((unsigned) T.blocks, blocks_of((size_t) S + 1))), dim3(kBlock), 0, st,
                       d_tab, S, (unsigned) T.blocks, (unsigned) total, d_pts, (const unsigned *) flag, (const unsigned *) pos,
                       d_idx, d_cap, d_pout, c.out_stride, d_offs);
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    const size_t offs_words = (size_t) S + 1 + (c.negative ? S : 0);
    WM_TRY(sac_fetch(ctx, w.h_round.p, d_offs, offs_words * 4));
    WM_HIP(ctx, hipStreamSynchronize(st));
    const unsigned *h_offs = w.h_round.as<unsigned>(), *h_ninl = h_offs + S + 1;
    for (unsigned k = 0; k <= S; ++k) c.offsets_out[k] = h_offs[k];
    const size_t kept = h_offs[S];
    if (c.stats)
        for (unsigned k = 0; k < S; ++k)
            if (h_fin[k].has) c.stats[k].n_inliers = c.negative ? h_ninl[k] : h_offs[k + 1] - h_offs[k];
    WM_TRY(finish(&ms));
    const size_t m = std::min(kept, c.cap);
    if (c.host_out) {
        if (m) WM_HIP(ctx, hipMemcpy(c.indices_out, d_idx, m * 4, hipMemcpyDeviceToHost));
        if (m && c.points_out) WM_HIP(ctx, hipMemcpy(c.points_out, d_pout, m * c.out_stride, hipMemcpyDeviceToHost));
    }
    return kept > c.cap ? WM_ERR_ARG : WM_OK;
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

int wm_sac_segment_batch(wm_ctx *ctx, const wm_sac_scan *scans, int n_scans, size_t stride, int mem, const wm_sac_params *p,
                         int negative, float *coefficients_out, int32_t *indices_out, size_t cap, void *points_out,
                         size_t out_stride, int out_mem, size_t *offsets_out, uint8_t *labels_out, int *status,
                         wm_sac_stats *stats, float *kernel_ms) {
    if (!ctx || n_scans < 0 || !scans || !status || !coefficients_out || !offsets_out ||
        (cap > 0 && !indices_out) || (points_out && (out_stride < 12 || (out_stride & 3))) ||
        !sac_args_ok(p, stride, mem, out_mem) || (unsigned long long) n_scans > WM_SAC_BATCH_MAX_SCANS)
        return WM_ERR_ARG;
    const unsigned S = (unsigned) n_scans;
    size_t total = 0;
    bool any = false;
    for (unsigned k = 0; k < S; ++k) {
        if ((scans[k].n > 0 && !scans[k].pts) || scans[k].n > WM_SAC_BATCH_MAX_POINTS) return WM_ERR_ARG;
        total += scans[k].n;
        if (total > WM_SAC_BATCH_MAX_POINTS) return WM_ERR_ARG;
        any = any || scans[k].n >= 3;
    }
    for (unsigned k = 0; k <= S; ++k) offsets_out[k] = 0;
    for (unsigned k = 0; k < S; ++k) status[k] = WM_NOT_CONVERGED;
    if (stats)
        for (unsigned k = 0; k < S; ++k) {
            stats[k] = wm_sac_stats{};
            stats[k].best_hypothesis = -1;
        }
    if (kernel_ms) *kernel_ms = 0.f;
    if (!any) {  // (no sample anywhere: no device is touched)
        if (labels_out && out_mem == WM_MEM_HOST && total) memset(labels_out, 0, total);
        return WM_OK;
    }
    const SacBatchCall c{scans, S, stride, mem, p, negative, coefficients_out, indices_out, cap, points_out,
                         points_out ? out_stride : 0, out_mem == WM_MEM_HOST, offsets_out, labels_out, status, stats, kernel_ms};
    return sac_batch(ctx, c);
}

}  // extern "C"
