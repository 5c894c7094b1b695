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
// ONE set of kernels and one host back (sac_call) serve both entry points, as in wm_ground.hip, wm_outlier.hip and
// wm_cluster.hip: the scans reach the kernels as a device table, or as tab == nullptr and the one scan by value in the
// kernel arguments (the single call: no table, no staging, nothing uploaded).  So every byte of scan k of a batch EQUALS
// the single call's for that scan alone -- `rounds` and the refit's bits included -- because the same code made it.
//   front      the single call: pack_cloud.  A batch: wm_scan_table.hpp's table and pack into batch positions.
//   a round    a row (SacRow) per LIVE scan, each with its own j0 and R: the batch's rows go up as a small table, the
//              single call's one row travels in the kernel arguments (SacRows).
//     k_sac_hypotheses   one lane per stream entry of the round, over all rows: indices -> three point loads -> plane ->
//                        validity; a float4 and a flag
//     k_sac_count        the hot kernel; its workgroups are bound to ONE row each.  A lane keeps kSacPts points in
//                        registers and loops over the row's planes, read through a wave-uniform index (scalar loads);
//                        per plane a ballot and a popcount per point slot, accumulated per workgroup in LDS; one integer
//                        atomicAdd per plane and workgroup at its end.  Integer counts: order-independent.  The points
//                        are read once per round.
//     one fetch of the round's (flag, count) pairs, 8 bytes an entry; the first round's has the finite counts in front
//   behind the rounds (SacScans: the scan table with a SacFin per scan, or one of each by value)
//     k_sac_models       a lane per scan: the model is entry best_j of the scan's stream, evaluated again
//     k_sac_sums         where a scan is refitted: the nine sums of the model's inliers as exact integer limbs
//                        (wm_bins.hpp's splitting) in bins of the call's own; k_sac_bins_sums adds a scan's bins in one
//                        fixed order.  One fetch of a SacOut per scan, the 3 x 3 eigenproblem on the host
//     k_sac_select (flags and labels) -> exclusive_scan -> k_sac_compact, and one fetch of the offsets.  A call
//                        without a refit reads the models from the device and has them back with this fetch.
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
// entry -- wherever it is evaluated (a round's lane; the lane that recomputes a scan's model behind the rounds).
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

// ------------------------------------------------------------------ the kernels of a round
struct SacRow {  // a live scan in a round
    unsigned long long j0;  // its first stream entry of the round
    unsigned scan, R;       // the scan; its entries of the round (>= 1)
    unsigned e0, cb0;       // the first entry's place in the round's arrays; its first count workgroup
    unsigned off, n;        // the scan's first batch position; its points
    unsigned nb, pad;       // its count workgroups (>= 1)
};

// The rows of a round: a table in device memory (a batch), or tab == nullptr and the one row by value (the single call:
// entry 0, workgroup 0 and position 0 are its own).  at(x, field): the row that owns entry or workgroup x.
struct SacRows {
    const SacRow *tab;
    unsigned L;
    SacRow one;
    template <class Field>
    __device__ __forceinline__ SacRow at(unsigned x, Field field) const {
        if (tab) return tab[cl_find(tab, L, x, field)];
        return one;
    }
};

// One lane per entry of the round (E of them), over all rows.  counts[e] = 0 for the count kernel behind it.
__global__ void __launch_bounds__(kBlock)
    k_sac_hypotheses(const float4 *__restrict__ pts, SacRows rows, unsigned E, unsigned long long seed, SacAxis ax,
                     float4 *__restrict__ planes, unsigned *__restrict__ flags, unsigned *__restrict__ counts) {
    const unsigned e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    const SacRow me = rows.at(e, [](const SacRow &r) { return r.e0; });
    float4 pl;
    const unsigned flag = sac_hypothesis(pts + me.off, me.n, seed, me.j0 + (e - me.e0), ax, pl);
    planes[e] = pl;
    flags[e] = flag;
    counts[e] = 0u;
}

// The hot kernel (sac_count_tiles).  A workgroup is bound to tiles of ONE row: the LDS counters and the one atomic per
// plane and workgroup are that scan's.  finite_out: the single call's first round counts its finite points here (a
// batch has them from the pack).
__global__ void __launch_bounds__(kBlock)
    k_sac_count(const float4 *__restrict__ pts, SacRows rows, const float4 *__restrict__ planes,
                const unsigned *__restrict__ flags, float thr, unsigned *__restrict__ counts, unsigned *__restrict__ finite_out) {
    const SacRow me = rows.at(blockIdx.x, [](const SacRow &r) { return r.cb0; });
    sac_count_tiles(pts + me.off, me.n, planes + me.e0, flags + me.e0, me.R, thr, counts + me.e0, blockIdx.x - me.cb0, me.nb,
                    finite_out);
}

// ------------------------------------------------------------------ the kernels behind the rounds
struct SacFin {  // a scan behind the rounds
    long long best_j;       // its model's stream entry, -1: no model
    unsigned refit, bin0;   // whether its sums are formed; its first bin
    unsigned nbins, has;    // min(kSacBins, its waves); whether `coef` holds its returned plane (else: SacOut's model)
    unsigned pad[2];
    float4 coef;
};

struct SacOut {  // what the host needs of a scan behind the rounds
    double sum[kSacComps];
    float4 model, p0;
    unsigned poison, pad[3];
};

// The scans of a call behind the rounds: the scan table and a SacFin per scan in device memory (a batch), or
// tab == nullptr and the one scan with its SacFin by value (the single call; a look-up in a table of one never reads
// the table, cl_find).  Of a ClScan only n, off, blk0 and aux0 (the scan's first label) are read.
struct SacScans {
    const ClScan *tab;
    const SacFin *fins;
    unsigned S;
    ClScan one;
    SacFin fin1;
    __device__ __forceinline__ ClScan scan(unsigned k) const {
        if (tab) return tab[k];
        return one;
    }
    __device__ __forceinline__ SacFin fin(unsigned k) const {
        if (tab) return fins[k];
        return fin1;
    }
};

// One lane per scan: the model is entry best_j of the scan's stream, evaluated again, and p0 its sample's first point
// (finite, since the entry was valid).
__global__ void __launch_bounds__(kBlock)
    k_sac_models(SacScans sc, const float4 *__restrict__ pts, unsigned long long seed, SacAxis ax, SacOut *__restrict__ out) {
    const unsigned k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= sc.S) return;
    float4 pl = make_float4(0.f, 0.f, 0.f, 0.f), p0 = pl;
    const long long bj = sc.fin(k).best_j;
    if (bj >= 0) {
        const ClScan me = sc.scan(k);
        (void) sac_hypothesis(pts + me.off, me.n, seed, (unsigned long long) bj, ax, pl);
        unsigned i[3];
        sac_sample(seed, (unsigned long long) bj, me.n, i);
        p0 = pts[me.off + i[0]];
    }
    out[k].model = pl;
    out[k].p0 = p0;
    out[k].poison = 0u;
}

// The refit's sums over the MODEL's inliers, relative to p0, over batch positions.  The workgroups are aligned to each
// scan's start (blk0), so a wave's number INSIDE its scan mod kSacBins is its bin, whatever else is in the call; the
// scan's bins start at bin0.
__global__ void __launch_bounds__(kBlock)
    k_sac_sums(SacScans sc, const SacOut *__restrict__ out, const float4 *__restrict__ pts, float thr,
               long long *__restrict__ bins) {
    const unsigned k = cl_by_block(sc.tab, sc.S, blockIdx.x);
    const SacFin f = sc.fin(k);
    if (!f.refit) return;  // (the whole workgroup)
    const ClScan me = sc.scan(k);
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

// A workgroup per scan: its bins into the nine doubles and the poison flag.  Thread b turns bin b's limbs into their
// values (bins_value: a bin's limbs are exact integers, so its value is a function of the inliers); thread c then adds
// component c's values in DOUBLE, bin 0 first, every add rounded.  The refit's bits depend on which wave fed which bin
// and on this order: tests/test_sac_pinned_gpu.py holds them to a record.  A bin that no wave fed is +0.0 and changes
// no sum: a scan of fewer than kSacBins waves has only its waves' bins.
__global__ void __launch_bounds__(kSacBins)
    k_sac_bins_sums(SacScans sc, const long long *__restrict__ bins, SacOut *__restrict__ out) {
    __shared__ double s_val[kSacComps][kSacBins];
    __shared__ unsigned s_poison;
    const unsigned k = blockIdx.x;
    const SacFin f = sc.fin(k);
    if (!f.refit) return;  // (the whole workgroup)
    if (threadIdx.x == 0u) s_poison = 0u;
    __syncthreads();
    if (threadIdx.x < f.nbins) {
        const long long *w = bins + ((size_t) f.bin0 + threadIdx.x) * kSacBinSize;
#pragma unroll
        for (int c = 0; c < kSacComps; ++c) s_val[c][threadIdx.x] = bins_value(w[c], w[kSacStride + c], w[2 * kSacStride + c]);
        if (w[kSacPoison] != 0ll) s_poison = 1u;  // (every writer writes 1)
    }
    __syncthreads();
    if (threadIdx.x < (unsigned) kSacComps) {
        double s = 0.0;
#pragma unroll 8
        for (unsigned b = 0; b < f.nbins; ++b) s += s_val[threadIdx.x][b];
        out[k].sum[threadIdx.x] = s;
    }
    if (threadIdx.x == 0u) out[k].poison = s_poison;
}

// The selection over batch positions with the scans' returned planes: the refit's, or where the call has no refit the
// model as k_sac_models left it.  flag: inlier, or with `negative` finite non-inlier; a scan without a model keeps
// nothing and its labels are NONE.  labels: the scans' n entries one after the other (aux0: the scan's first label).
// ninl != nullptr: the scans' inliers are counted (integers).
__global__ void __launch_bounds__(kBlock)
    k_sac_select(SacScans sc, const SacOut *__restrict__ out, const float4 *__restrict__ pts, float thr, int negative,
                 unsigned *__restrict__ flag, unsigned char *__restrict__ labels, unsigned *__restrict__ ninl) {
    const unsigned k = cl_by_block(sc.tab, sc.S, blockIdx.x);
    const ClScan me = sc.scan(k);
    const SacFin f = sc.fin(k);
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    const bool has = f.best_j >= 0;
    bool in = false, finite = false;
    if (i < me.n) {
        const float4 pl = f.has ? f.coef : out[k].model;
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
    k_sac_compact(SacScans sc, unsigned blocks, unsigned total, const float4 *__restrict__ pts,
                  const unsigned *__restrict__ flag, const unsigned *__restrict__ pos, int *__restrict__ idx_out, size_t cap,
                  unsigned char *__restrict__ pout, size_t out_stride, unsigned *__restrict__ offs) {
    const size_t g = (size_t) blockIdx.x * kBlock + threadIdx.x;
    if (g <= sc.S) offs[g] = pos[g < sc.S ? sc.scan((unsigned) g).off : total];
    if (blockIdx.x >= blocks) return;
    const ClScan me = sc.scan(cl_by_block(sc.tab, sc.S, blockIdx.x));
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
    DevBuf pts;            // the packed clouds, batch positions
    DevBuf round;          // [7 S words: the boxes (a batch's pack) and finite counts][E flags][E counts] ... [E planes]
    DevBuf bins;           // the refitted scans' bins
    DevBuf flag, pos;      // the selection's scan
    DevBuf idx, labels;    // host outputs on their way
    DevBuf pout;           // the points of a caller in host memory on their way
    DevBuf out;            // [S SacOut][S + 1 offsets][S inlier counts]
    DevBuf rows, fin;      // a batch: the round's table, the scans' SacFin
    PairStage stage;       // a batch's scan table and host clouds up (wm_stage.hpp)
    PinnedBuf h_round, h_out;
    PinnedBuf h_rows, h_fin;
};

void sac_release(wm_ctx *ctx) {
    SacWs *w = static_cast<SacWs *>(ctx->sac);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts, &w->round, &w->bins, &w->flag, &w->pos, &w->idx, &w->labels, &w->pout, &w->out, &w->rows,
                      &w->fin};
    for (DevBuf *b : bufs) b->release();
    w->stage.release();
    PinnedBuf *pins[] = {&w->h_round, &w->h_out, &w->h_rows, &w->h_fin};
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

// A fetch: small ones by fast_fetch's one workgroup, large ones (a long round of many scans) by the copy engine.
int sac_fetch(wm_ctx *ctx, void *dst_pinned, const void *src_dev, size_t bytes) {
    if (bytes <= ((size_t) 64 << 10)) return fast_fetch(ctx, dst_pinned, src_dev, bytes);
    WM_HIP(ctx, hipMemcpyAsync(dst_pinned, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

// A call of either entry point: wm_sac_segment_batch's arguments, which wm_sac_segment fills for its one scan.
struct SacCall {
    bool single;  // wm_sac_segment: the scan by value, no table; no labels without a model; timed only with stats
    const wm_sac_scan *scans;
    unsigned S;
    size_t stride;
    int mem;
    const wm_sac_params *p;
    int negative;
    float *coefficients_out;  // 4 S
    int32_t *indices_out;
    size_t cap;
    void *points_out;
    size_t out_stride;
    bool host_out;
    size_t *offsets_out;  // S + 1
    uint8_t *labels_out;
    int *status;          // S, WM_NOT_CONVERGED on entry
    wm_sac_stats *stats;
    float *kernel_ms;
};

// Either entry point (arguments checked, the outputs' defaults written, at least one scan of n >= 3).  Launches and
// host waits: the front (a batch: upload; pack), per round of the longest-living scan two launches and one fetch (a
// batch: the round's table up), then the models and, where a scan is refitted, the sums with one fetch of their own (a
// batch: the coefficients up), select / scan / compact and one fetch of the offsets -- whatever the number of scans.
// The single call uploads nothing and waits once per round, once for the refit and once at the end.
int sac_call(wm_ctx *ctx, const SacCall &c) {
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
    const bool timed = !c.single || c.stats;  // (a batch's PairStage::submit records ev_a)

    // ---- the scans' walks and the sizes of the first round.  A scan of n < 3 has no sample: it gets no batch position
    // and no workgroup (n = 0 in the table)
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
    const size_t out_bytes = (size_t) S * sizeof(SacOut);  // (behind the SacOuts: S + 1 offsets, S inlier counts)
    WM_HIP(ctx, w.h_round.reserve(((size_t) S + 2 * E0) * 4));
    WM_HIP(ctx, w.h_rows.reserve((live.size() + 1) * sizeof(SacRow)));
    WM_HIP(ctx, w.h_fin.reserve((size_t) S * sizeof(SacFin)));
    WM_HIP(ctx, w.out.reserve(out_bytes + (2 * (size_t) S + 1) * 4));
    WM_HIP(ctx, w.h_out.reserve(out_bytes + (2 * (size_t) S + 1) * 4));
    // ---- the front: the packed points, the scan table (aux0 is a scan's first label, which counts a tiny scan's points)
    ScanTable T;
    ClScan one{};
    if (c.single) {  // no table on the device: the one scan owns position 0, workgroup 0 and label 0 of everything
        WM_HIP(ctx, w.pts.reserve(c.scans[0].n * sizeof(float4)));
        WM_HIP(ctx, w.round.reserve(round_bytes));
        if (timed) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
        WM_TRY(pack_cloud(ctx, c.scans[0].pts, c.scans[0].n, c.stride, c.mem, w.pts.as<float4>()));
        WM_HIP(ctx, hipMemsetAsync(w.round.as<unsigned>() + 6, 0, 4, st));  // (the finite points: the first round's count)
        one.n = (unsigned) c.scans[0].n;
        T.tab = &one;
        T.S = 1;
        T.total = one.n;
        T.blocks = blocks_of(one.n);
    } else {
        WM_HIP(ctx, w.rows.reserve((live.size() + 1) * sizeof(SacRow)));
        WM_HIP(ctx, w.fin.reserve((size_t) S * sizeof(SacFin)));
        WM_TRY(scan_table_pack(ctx, w.stage, rows_in.data(), S, c.stride, c.mem, w.pts, w.round, round_bytes, &T));
        // the labels' places; the table goes up again with them (the pack did not read them)
        size_t at = 0;
        for (unsigned k = 0; k < S; ++k) {
            T.tab[k].aux0 = (unsigned) at;
            at += c.scans[k].n;
        }
        WM_HIP(ctx, hipMemcpyAsync(w.stage.up.dev.p, w.stage.up.host.p, T.table_bytes, hipMemcpyHostToDevice, st));
    }
    const size_t total = T.total;
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
        SacRows rows{nullptr, L, h_rows[0]};
        if (!c.single) {
            WM_HIP(ctx, hipMemcpyAsync(w.rows.p, h_rows, ((size_t) L + 1) * sizeof(SacRow), hipMemcpyHostToDevice, st));
            rows.tab = w.rows.as<SacRow>();
        }
        hipLaunchKernelGGL(k_sac_hypotheses, dim3(blocks_of(E)), dim3(kBlock), 0, st, d_pts, rows, E, seed, ax, d_planes, d_flags,
                           d_counts);
        hipLaunchKernelGGL(k_sac_count, dim3(cb), dim3(kBlock), 0, st, d_pts, rows, (const float4 *) d_planes,
                           (const unsigned *) d_flags, thr, d_counts,
                           c.single && round == 0 ? d_words + 6 : (unsigned *) nullptr);
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
    auto finish = [&]() -> int {  // (the stream has been waited for)
        float ms = 0.f;
        if (timed && hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b) != hipSuccess) ms = 0.f;
        if (c.kernel_ms) *c.kernel_ms = ms;
        if (c.stats)
            for (unsigned k = 0; k < S; ++k)
                if (c.scans[k].n >= 3) c.stats[k].kernel_ms = ms;
        if (c.host_out && d_labels) WM_HIP(ctx, hipMemcpy(c.labels_out, d_labels, label_total, hipMemcpyDeviceToHost));
        return WM_OK;
    };
    if (!any_model) {  // every slice is empty; a batch's labels are NONE, the single call writes none
        if (c.single) d_labels = nullptr;
        if (d_labels) WM_HIP(ctx, hipMemsetAsync(d_labels, 0, label_total, st));
        if (timed) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
        WM_HIP(ctx, hipStreamSynchronize(st));
        return finish();
    }

    // ---- the models again from their entries; where a scan is refitted, its sums and one fetch of the SacOuts
    SacScans sc{T.d_tab, w.fin.as<SacFin>(), S, one, h_fin[0]};
    SacOut *d_out = w.out.as<SacOut>();
    const SacOut *h_out = w.h_out.as<SacOut>();
    if (sc.tab) WM_HIP(ctx, hipMemcpyAsync(w.fin.p, h_fin, (size_t) S * sizeof(SacFin), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sac_models, dim3(blocks_of(S)), dim3(kBlock), 0, st, sc, d_pts, seed, ax, d_out);
    if (n_bins) {
        WM_HIP(ctx, w.bins.reserve(n_bins * kSacBinSize * sizeof(long long)));
        long long *d_bins = w.bins.as<long long>();
        WM_HIP(ctx, hipMemsetAsync(d_bins, 0, n_bins * kSacBinSize * sizeof(long long), st));
        hipLaunchKernelGGL(k_sac_sums, dim3((unsigned) T.blocks), dim3(kBlock), 0, st, sc, (const SacOut *) d_out, d_pts, thr,
                           d_bins);
        hipLaunchKernelGGL(k_sac_bins_sums, dim3(S), dim3(kSacBins), 0, st, sc, (const long long *) d_bins, d_out);
    }
    WM_HIP(ctx, hipGetLastError());
    // the SacOuts at home: the scans' returned planes (the refit on the host, wm_sac_walk.hpp) and what the caller gets
    auto planes_home = [&]() {
        for (unsigned k = 0; k < S; ++k) {
            SacFin &f = h_fin[k];
            if (f.best_j < 0) continue;
            const SacOut &o = h_out[k];
            const float model[4] = {o.model.x, o.model.y, o.model.z, o.model.w};
            const float p0[3] = {o.p0.x, o.p0.y, o.p0.z};
            float coef[4] = {model[0], model[1], model[2], model[3]};
            int refined = 0;
            if (f.refit) {
                if (sac_plane_from_sums(o.sum, o.poison != 0u, p0, (double) walk[k].best, model, coef)) refined = 1;
                else memcpy(coef, model, sizeof(coef));
            }
            f.has = 1u;
            f.coef = make_float4(coef[0], coef[1], coef[2], coef[3]);
            memcpy(c.coefficients_out + 4 * (size_t) k, coef, sizeof(coef));
            c.status[k] = WM_OK;
            if (c.stats) {
                c.stats[k].n_inliers_model = (size_t) walk[k].best;
                memcpy(c.stats[k].model_coefficients, model, sizeof(model));
                c.stats[k].refined = refined;
            }
        }
    };
    if (n_bins) {  // the selection takes the planes from the SacFins; else it reads the models where k_sac_models left them
        WM_TRY(sac_fetch(ctx, w.h_out.p, d_out, out_bytes));
        planes_home();
        sc.fin1 = h_fin[0];
        if (sc.tab) WM_HIP(ctx, hipMemcpyAsync(w.fin.p, h_fin, (size_t) S * sizeof(SacFin), hipMemcpyHostToDevice, st));
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
    unsigned *d_offs = reinterpret_cast<unsigned *>(d_out + S), *d_ninl = d_offs + S + 1;
    if (c.negative) WM_HIP(ctx, hipMemsetAsync(d_ninl, 0, (size_t) S * 4, st));
    if (d_labels && tiny) WM_HIP(ctx, hipMemsetAsync(d_labels, 0, label_total, st));  // (no workgroup writes a tiny scan's)
    hipLaunchKernelGGL(k_sac_select, dim3((unsigned) T.blocks), dim3(kBlock), 0, st, sc, (const SacOut *) d_out, d_pts, thr,
                       c.negative, flag, d_labels, c.negative ? d_ninl : (unsigned *) nullptr);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, flag, total, pos));
    hipLaunchKernelGGL(k_sac_compact, dim3(std::max((unsigned) T.blocks, blocks_of((size_t) S + 1))), dim3(kBlock), 0, st, sc,
                       (unsigned) T.blocks, (unsigned) total, d_pts, (const unsigned *) flag, (const unsigned *) pos, d_idx, d_cap,
                       d_pout, c.out_stride, d_offs);
    WM_HIP(ctx, hipGetLastError());
    // kernel_ms ends behind a batch's last launch and behind the single call's last fetch.  That fetch: the offsets (and
    // the inlier counts), behind the SacOuts where these have not come home yet
    if (timed && !c.single) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    const size_t from = n_bins ? out_bytes : 0, offs_words = (size_t) S + 1 + (c.negative ? S : 0);
    WM_TRY(sac_fetch(ctx, w.h_out.as<unsigned char>() + from, w.out.as<unsigned char>() + from,
                     out_bytes - from + offs_words * 4));
    if (timed && c.single) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (!n_bins) planes_home();
    const unsigned *h_offs = reinterpret_cast<const unsigned *>(h_out + S), *h_ninl = h_offs + S + 1;
    for (unsigned k = 0; k <= S; ++k) c.offsets_out[k] = h_offs[k];
    const size_t kept = h_offs[S];
    if (c.stats)
        for (unsigned k = 0; k < S; ++k)
            if (h_fin[k].best_j >= 0) c.stats[k].n_inliers = c.negative ? h_ninl[k] : h_offs[k + 1] - h_offs[k];
    WM_TRY(finish());
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
    const wm_sac_scan scan{pts, n};
    size_t offs[2] = {0, 0};
    int status = WM_NOT_CONVERGED;
    const SacCall c{true, &scan, 1, stride, mem, p, 0, coefficients_out, indices_out, cap, nullptr, 0, out_mem == WM_MEM_HOST,
                    offs, labels_out, &status, stats, nullptr};
    const int rc = sac_call(ctx, c);
    *n_out = offs[1];
    return rc == WM_OK ? status : rc;
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
    const SacCall c{false, scans, S, stride, mem, p, negative, coefficients_out, indices_out, cap, points_out,
                    points_out ? out_stride : 0, out_mem == WM_MEM_HOST, offsets_out, labels_out, status, stats, kernel_ms};
    return sac_call(ctx, c);
}

}  // extern "C"
