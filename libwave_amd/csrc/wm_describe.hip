// wm_describe.hip -- cluster boxes on the device (wm_cluster_boxes): per cluster of a member list the count, the
// axis-aligned box, the centroid, the covariance's eigenvalues and axes, and PCL's oriented box.  The rule is stated in
// include/wavematch.h ("cluster boxes"); the checker is tests/boxes_reference.py.
//
// The work is three segmented reductions over the member list with a per-cluster step between them:
//   k_box_check            the offsets' rule (ascending, first 0, last n_members), counted into err[0]; the first
//                          pass's accumulators set to their identities; per tile of the member list the cluster of
//                          its first member (tile_c), written by that cluster's own lane
//   k_box_pass<PassAabb>   min / max of the orderable float keys, the finite count, the non-finite flag
//   k_box_mid              n, flags and the AABB into the box; WM_BOX_RANGE
//   k_box_pass<PassSums>   the nine terms of d = p - aabb_min as three 40-bit limbs of trunc(t * 2^56) each (wm_bins.hpp)
//   k_box_eig              one cluster per lane: centroid, covariance, Jacobi, the order and signs of the axes
//   k_box_pass<PassObb>    min / max of the orderable keys of the three projections (doubles)
//   k_box_obb              the oriented box
// The AABB has to be complete before the sums (they are taken from its corner) and the axes before the projections:
// three streaming passes, not two.  Seven launches, two memsets and one fetch, whatever n_clusters and n_members are.
//
// k_box_pass: a workgroup owns a fixed tile of kBoxTile members, a wave four chunks of 64 of them, a lane one member
// per chunk.  Nobody searches `offsets`: the tile's clusters are tile_c[t] ... tile_c[t + 1], their offsets are read
// once, coalesced, each cluster marks the member it begins at in LDS (the largest mark stays where empty clusters share
// a place), and a member's cluster is the running maximum of the marks up to it -- a scan inside each chunk and the
// chunks' maxima across them.  (A binary search per member, ten dependent loads behind two of eighteen for the tile's
// range, made each pass 25-47 us on 270 000 members: latency, with one workgroup per CU.)
// Inside a chunk the values are combined by a segmented scan over the lanes (a lane joins the
// lane d below it iff both are in the same cluster: the members of a cluster are contiguous); the last lane of each
// run holds the run's total.  Every combination is an integer add, min, max or or, so the total does not depend on how
// the members are grouped.  Where the total goes:
//   the cluster lies wholly inside the chunk      a plain store by that lane, the cluster's only writer
//   else                                          into one of 17 slots of the workgroup's LDS (slot 0: the cluster that
//                                                 began before the tile; slot 1 + k: the one cluster that begins in
//                                                 chunk k and leaves it), by LDS integer atomics
// and after a barrier each used slot is stored plainly when its cluster lies wholly inside the tile, and goes to the
// cluster's accumulators by 64-bit integer atomics at agent scope otherwise: at most two clusters of a tile, 1 + n / 1024
// atomics per word for one cluster of n members, none at all for clusters that no tile edge cuts.  No lane waits for
// another wave: no flags, no tickets, no persistent kernel.
// Invalid input never leads a read astray: the passes do not run when err[0] is set (so tile_c is read only when every
// entry of it was written from a valid list), k_box_check reads entries 0 ... n_clusters of `offsets` and writes tiles
// below the tile count only, and an index outside [0, n) is counted (err[1]) and its member skipped.
#include <string.h>

#include "wm_bins.hpp"

#include <algorithm>
#include <cmath>

namespace wm {

namespace {

typedef unsigned long long u64;

constexpr int kBoxTile = 1024;                    // members of a workgroup's tile
constexpr int kBoxChunk = 64;                     // ... of one step of a wave
constexpr int kBoxChunks = kBoxTile / kBoxChunk;  // 16
constexpr int kBoxWaves = kBlock / 64;
constexpr int kBoxSlots = kBoxChunks + 1;
constexpr int kBoxTerms = 9;                      // x y z xx xy xz yy yz zz
constexpr u64 kLimbMask = (1ull << 40) - 1ull;
static_assert(kBoxChunks % kBoxWaves == 0 && kBinLimbs == 3, "chunks per wave; three limbs per term");
static_assert(sizeof(wm_cluster_box) == 128, "wm_cluster_box is 128 bytes");

enum BoxOp { kAdd, kMin, kMax, kOr };

__device__ __forceinline__ u64 box_ident(int op) { return op == kMin ? ~0ull : 0ull; }
__device__ __forceinline__ u64 box_combine(int op, u64 a, u64 b) {
    return op == kAdd ? a + b : op == kMin ? (a < b ? a : b) : op == kMax ? (a > b ? a : b) : (a | b);
}
// *p = combine(*p, v) by an integer atomic (LDS or global: the address space follows the pointer)
__device__ __forceinline__ void box_atomic(int op, u64 *p, u64 v) {
    if (op == kAdd)
        (void) atomicAdd(p, v);
    else if (op == kMin)
        (void) atomicMin(p, v);
    else if (op == kMax)
        (void) atomicMax(p, v);
    else
        (void) atomicOr(p, v);
}

// float / double <-> unsigned whose unsigned order is the number's order (-0 below +0)
__device__ __forceinline__ unsigned box_key(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float box_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ u64 box_key(double d) {
    const u64 b = (u64) __double_as_longlong(d);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double box_unkey(u64 k) {
    return __longlong_as_double((long long) ((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

struct BoxList {
    const unsigned char *pts;  // n records of `stride` bytes
    unsigned n, stride;
    const int *indices;        // nullptr: member e is record e
    unsigned n_members;
    const unsigned *offsets;   // n_clusters + 1
    unsigned n_clusters;
};

// member e: 0 = not a record of the cloud, 1 = a non-finite record, 2 = finite (x y z set)
__device__ __forceinline__ int box_member(const BoxList &L, unsigned e, float &x, float &y, float &z, unsigned *err, bool count) {
    const unsigned idx = L.indices ? (unsigned) L.indices[e] : e;
    if (idx >= L.n) {
        if (count) (void) atomicAdd(err + 1, 1u);
        return 0;
    }
    const float *p = reinterpret_cast<const float *>(L.pts + (size_t) idx * L.stride);
    x = p[0];
    y = p[1];
    z = p[2];
    return (isfinite(x) && isfinite(y) && isfinite(z)) ? 2 : 1;
}

// ---- the three passes: W words per cluster, word k combined by op(k); terms() = one member's words
struct PassAabb {  // [0..2] min keys, [3..5] max keys, [6] finite members, [7] flags
    static constexpr int W = 8;
    static constexpr bool kLimbs = false, kCountsErrors = true;
    static __device__ __forceinline__ int op(int k) { return k < 3 ? kMin : k < 6 ? kMax : k == 6 ? kAdd : kOr; }
    static __device__ __forceinline__ void terms(const wm_cluster_box *, unsigned, int state, float x, float y, float z,
                                                 u64 (&v)[W]) {
        const bool in = state == 2;  // (selects, not branches: every word is written once)
        v[0] = in ? (u64) box_key(x) : ~0ull;
        v[1] = in ? (u64) box_key(y) : ~0ull;
        v[2] = in ? (u64) box_key(z) : ~0ull;
        v[3] = in ? (u64) box_key(x) : 0ull;
        v[4] = in ? (u64) box_key(y) : 0ull;
        v[5] = in ? (u64) box_key(z) : 0ull;
        v[6] = in ? 1ull : 0ull;
        v[7] = state == 1 ? (u64) WM_BOX_NONFINITE : 0ull;
    }
};

struct PassSums {  // word limb * 9 + term: the limbs of trunc(term * 2^56)
    static constexpr int W = kBinLimbs * kBoxTerms;
    static constexpr bool kLimbs = true, kCountsErrors = false;
    static __device__ __forceinline__ int op(int) { return kAdd; }
    static __device__ __forceinline__ void terms(const wm_cluster_box *boxes, unsigned c, int state, float x, float y, float z,
                                                 u64 (&v)[W]) {
        if (state != 2) return;
        const wm_cluster_box &b = boxes[c];
        if (b.flags & WM_BOX_RANGE) return;
        const double dx = (double) x - (double) b.aabb_min[0], dy = (double) y - (double) b.aabb_min[1],
                     dz = (double) z - (double) b.aabb_min[2];
        const double t[kBoxTerms] = {dx, dy, dz, dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz};
#pragma unroll
        for (int j = 0; j < kBoxTerms; ++j) {
            long long l[kBinLimbs];
            bins_split(t[j], l);  // (0 <= t < 2^40: every limb is >= 0)
#pragma unroll
            for (int k = 0; k < kBinLimbs; ++k) v[k * kBoxTerms + j] = (u64) l[k];
        }
    }
};

struct PassObb {  // [0..2] min keys, [3..5] max keys of the projections on the returned axes
    static constexpr int W = 6;
    static constexpr bool kLimbs = false, kCountsErrors = false;
    static __device__ __forceinline__ int op(int k) { return k < 3 ? kMin : kMax; }
    static __device__ __forceinline__ void terms(const wm_cluster_box *boxes, unsigned c, int state, float x, float y, float z,
                                                 u64 (&v)[W]) {
        if (state != 2) return;
        const wm_cluster_box &b = boxes[c];
        if (b.flags & WM_BOX_RANGE) return;
        const double ex = (double) x - (double) b.centroid[0], ey = (double) y - (double) b.centroid[1],
                     ez = (double) z - (double) b.centroid[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double s = (ex * (double) b.axes[3 * k] + ey * (double) b.axes[3 * k + 1]) + ez * (double) b.axes[3 * k + 2];
            v[k] = v[3 + k] = box_key(s);
        }
    }
};

// the value of the lane D below in the same row of 16 lanes (DPP row_shr: no LDS crossbar); lanes without one keep their own
template <int D>
__device__ __forceinline__ unsigned box_row_shr(unsigned x) {
    return (unsigned) __builtin_amdgcn_update_dpp((int) x, (int) x, 0x110 + D, 0xF, 0xF, false);
}
template <int D>
__device__ __forceinline__ u64 box_row_shr(u64 x) {
    return ((u64) box_row_shr<D>((unsigned) (x >> 32)) << 32) | (u64) box_row_shr<D>((unsigned) x);
}
// one step of the segmented scan inside rows of 16 lanes
template <class P, int D>
__device__ __forceinline__ void box_row_step(unsigned c, u64 (&v)[P::W], unsigned lane) {
    const unsigned cd = box_row_shr<D>(c);
    const bool join = (lane & 15u) >= (unsigned) D && cd == c;
#pragma unroll
    for (int k = 0; k < P::W; ++k) {
        const u64 t = box_row_shr<D>(v[k]);
        if (join) v[k] = box_combine(P::op(k), v[k], t);
    }
}

template <class P>
__global__ void __launch_bounds__(kBlock)
    k_box_pass(BoxList L, const unsigned *__restrict__ tile_c, unsigned tiles, const wm_cluster_box *__restrict__ boxes,
               u64 *__restrict__ acc, unsigned *__restrict__ err) {
    constexpr int W = P::W;
    constexpr int kPerWave = kBoxChunks / kBoxWaves;
    __shared__ u64 slot_val[kBoxSlots * W];
    __shared__ unsigned slot_c[kBoxSlots];
    __shared__ unsigned head[kBoxTile];        // per member of the tile: the last cluster that begins there, 0 for none
    __shared__ unsigned chunk_max[kBoxChunks];
    if (err[0] != 0u) return;  // (uniform: the offsets are not a partition of the list)
    const unsigned tile_base = blockIdx.x * (unsigned) kBoxTile;
    const unsigned tile_end = min(tile_base + (unsigned) kBoxTile, L.n_members);
    const unsigned tile_len = tile_end - tile_base;
    // the tile's clusters: c_lo holds the tile's first member (k_box_check's table); every later one begins inside
    const unsigned c_lo = tile_c[blockIdx.x];
    const unsigned c_up = blockIdx.x + 1u < tiles ? tile_c[blockIdx.x + 1u] : L.n_clusters - 1u;
    for (unsigned i = threadIdx.x; i < (unsigned) (kBoxSlots * W); i += kBlock) slot_val[i] = box_ident(P::op((int) (i % W)));
    if (threadIdx.x < (unsigned) kBoxSlots) slot_c[threadIdx.x] = kNoIdx;
    for (unsigned i = threadIdx.x; i < (unsigned) kBoxTile; i += kBlock) head[i] = i == 0u ? c_lo : 0u;
    __syncthreads();
    // one coalesced read of the tile's offsets instead of a search per member: cluster c marks where it begins (empty
    // clusters share a place: the largest stays), and a member's cluster is the largest mark at or before it
    for (unsigned c = c_lo + 1u + threadIdx.x; c <= c_up && c > c_lo; c += kBlock) {
        const unsigned pos = L.offsets[c] - tile_base;  // (an offset before the tile wraps and fails the test)
        if (pos >= 1u && pos < tile_len) (void) atomicMax(&head[pos], c);
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned mark[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {  // the running maximum inside each chunk
        const unsigned chunk = wave * (unsigned) kPerWave + (unsigned) i;
        unsigned h = head[chunk * (unsigned) kBoxChunk + lane];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(h, d, 64);
            if (lane >= (unsigned) d) h = max(h, t);
        }
        mark[i] = h;
        if (lane == 63u) chunk_max[chunk] = h;
    }
    __syncthreads();

#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
        const unsigned chunk = wave * (unsigned) kPerWave + (unsigned) i;
        const unsigned chunk_base = tile_base + chunk * (unsigned) kBoxChunk;
        if (chunk_base >= tile_end) break;  // (uniform in the wave; the barrier is behind the loop)
        const unsigned e = chunk_base + lane;
        const bool valid = e < tile_end;
        unsigned before = 0u;  // the largest mark of the chunks in front (uniform)
        for (unsigned j = 0; j < chunk; ++j) before = max(before, chunk_max[j]);
        const unsigned c = valid ? max(mark[i], before) : kNoIdx;
        u64 v[W];
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = box_ident(P::op(k));
        if (valid) {
            float x = 0.f, y = 0.f, z = 0.f;
            const int state = box_member(L, e, x, y, z, err, P::kCountsErrors);
            P::terms(boxes, c, state, x, y, z, v);
        }
        // segmented inclusive scan: a lane joins the lane d below it iff the same cluster (a cluster's members are
        // contiguous).  Inside rows of 16 lanes by DPP shifts (vector ALU rate); the four rows' totals then by two steps
        // through the LDS crossbar.  (All six steps as shuffles made the sums pass crossbar-bound: 27 64-bit words x 6.)
        box_row_step<P, 1>(c, v, lane);
        box_row_step<P, 2>(c, v, lane);
        box_row_step<P, 4>(c, v, lane);
        box_row_step<P, 8>(c, v, lane);
#pragma unroll
        for (int step = 0; step < 2; ++step) {
            // rows 1 and 3 take the last lane of the row below; then rows 2 and 3 lane 31, which by now holds rows 0-1
            const int src = step == 0 ? (int) ((lane & ~31u) + 15u) : 31;
            const bool upper = step == 0 ? (lane & 16u) != 0u : (lane & 32u) != 0u;
            const unsigned cs = __shfl(c, src, 64);
            const bool join = upper && cs == c;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const u64 t = __shfl(v[k], src, 64);
                if (join) v[k] = box_combine(P::op(k), v[k], t);
            }
        }
        const unsigned c_next = __shfl_down(c, 1, 64);
        if (valid && (lane == 63u || c_next != c)) {  // the last lane of a run holds its total
            const unsigned rs = L.offsets[c], re = L.offsets[c + 1u];
            if (rs >= chunk_base && re <= chunk_base + (unsigned) kBoxChunk) {
#pragma unroll
                for (int k = 0; k < W; ++k) acc[(size_t) c * W + k] = v[k];
            } else {
                const unsigned s = rs < tile_base ? 0u : 1u + (rs - tile_base) / (unsigned) kBoxChunk;
                slot_c[s] = c;
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (v[k] != box_ident(P::op(k))) box_atomic(P::op(k), &slot_val[s * W + k], v[k]);
            }
        }
    }
    __syncthreads();
    if (P::kLimbs) {  // carries: a tile hands on limbs below 2^40, so 2^21 tiles fit a 64-bit word
        if (threadIdx.x < (unsigned) (kBoxSlots * kBoxTerms)) {
            u64 *p = slot_val + (threadIdx.x / kBoxTerms) * W + threadIdx.x % kBoxTerms;
            u64 l0 = p[0], l1 = p[kBoxTerms], l2 = p[2 * kBoxTerms];
            l1 += l0 >> 40;
            l2 += l1 >> 40;
            p[0] = l0 & kLimbMask;
            p[kBoxTerms] = l1 & kLimbMask;
            p[2 * kBoxTerms] = l2;
        }
        __syncthreads();
    }
    for (unsigned i = threadIdx.x; i < (unsigned) (kBoxSlots * W); i += kBlock) {
        const unsigned s = i / W;
        const int k = (int) (i % W);
        const unsigned c = slot_c[s];
        if (c == kNoIdx) continue;
        const u64 val = slot_val[i];
        if (L.offsets[c] >= tile_base && L.offsets[c + 1u] <= tile_base + (unsigned) kBoxTile)
            acc[(size_t) c * W + k] = val;
        else if (val != box_ident(P::op(k)))
            box_atomic(P::op(k), &acc[(size_t) c * W + k], val);
    }
}

// offsets[0] == 0, ascending, offsets[n_clusters] == n_members: every breach counted; the AABB pass's identities; and
// tile_c[t] = the cluster that holds member t * kBoxTile, written by that cluster's lane (a valid list has exactly one
// such cluster per tile; with an invalid one the passes do not run and the table is not read)
__global__ void __launch_bounds__(kBlock)
    k_box_check(const unsigned *__restrict__ off, unsigned n_clusters, unsigned n_members, u64 *__restrict__ acc,
                unsigned *__restrict__ tile_c, unsigned tiles, unsigned *__restrict__ err) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    if (c > n_clusters) return;
    bool bad = false;
    if (c < n_clusters) bad = off[c] > off[c + 1u];
    if (c == 0u) bad = bad || off[0] != 0u;
    if (c == n_clusters) bad = bad || off[c] != n_members;
    if (bad) (void) atomicAdd(err, 1u);
    if (c < n_clusters) {
#pragma unroll
        for (int k = 0; k < PassAabb::W; ++k) acc[(size_t) c * PassAabb::W + k] = box_ident(PassAabb::op(k));
        const unsigned lo = off[c], hi = off[c + 1u];
        if (lo < hi)
            for (unsigned t = lo / (unsigned) kBoxTile + (lo % (unsigned) kBoxTile != 0u ? 1u : 0u);
                 t < tiles && (u64) t * (u64) kBoxTile < (u64) hi; ++t)
                tile_c[t] = c;
    }
}

// n, flags and the AABB; every other field zero
__global__ void __launch_bounds__(kBlock)
    k_box_mid(const u64 *__restrict__ acc, unsigned n_clusters, wm_cluster_box *__restrict__ boxes,
              const unsigned *__restrict__ err) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_clusters || err[0] != 0u) return;
    const u64 *a = acc + (size_t) c * PassAabb::W;
    wm_cluster_box b;
    memset(&b, 0, sizeof(b));
    b.n = (unsigned) a[6];
    b.flags = (unsigned) a[7];
    if (b.n == 0u) {
        b.flags |= WM_BOX_EMPTY;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b.aabb_min[k] = box_unkey((unsigned) a[k]);
            b.aabb_max[k] = box_unkey((unsigned) a[3 + k]);
            if ((double) b.aabb_max[k] - (double) b.aabb_min[k] >= 1048576.0) b.flags |= WM_BOX_RANGE;
        }
    }
    boxes[c] = b;
}

// one cluster per lane: centroid, covariance, eigenvalues and axes; the OBB pass's identities
__global__ void __launch_bounds__(kBlock)
    k_box_eig(const u64 *__restrict__ sums, unsigned n_clusters, wm_cluster_box *__restrict__ boxes, u64 *__restrict__ acc,
              const unsigned *__restrict__ err) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_clusters || err[0] != 0u) return;
#pragma unroll
    for (int k = 0; k < PassObb::W; ++k) acc[(size_t) c * PassObb::W + k] = box_ident(PassObb::op(k));
    wm_cluster_box &b = boxes[c];
    const unsigned n = b.n;
    if (n == 0u || (b.flags & WM_BOX_RANGE)) return;
    double S[kBoxTerms];
#pragma unroll
    for (int j = 0; j < kBoxTerms; ++j) {  // the canonical limbs of the total, then the one rounding to double
        const u64 *p = sums + (size_t) c * PassSums::W + j;
        u64 l0 = p[0], l1 = p[kBoxTerms], l2 = p[2 * kBoxTerms];
        l1 += l0 >> 40;
        l2 += l1 >> 40;
        S[j] = bins_value((long long) (l0 & kLimbMask), (long long) (l1 & kLimbMask), (long long) l2);
    }
    const double nd = (double) n;
    const double m[3] = {S[0] / nd, S[1] / nd, S[2] / nd};
#pragma unroll
    for (int k = 0; k < 3; ++k) b.centroid[k] = (float) ((double) b.aabb_min[k] + m[k]);
    double A[9], w[3], V[9];
    A[0] = S[3] / nd - m[0] * m[0];
    A[1] = A[3] = S[4] / nd - m[0] * m[1];
    A[2] = A[6] = S[5] / nd - m[0] * m[2];
    A[4] = S[6] / nd - m[1] * m[1];
    A[5] = A[7] = S[7] / nd - m[1] * m[2];
    A[8] = S[8] / nd - m[2] * m[2];
    jacobi3(A, w, V);
    // (value, column) triples, clamped at 0 and put in descending order; equal values keep the order x, y, z
    double e0 = fmax(w[0], 0.0), e1 = fmax(w[1], 0.0), e2 = fmax(w[2], 0.0);
    double a0[3] = {V[0], V[3], V[6]}, a1[3] = {V[1], V[4], V[7]}, a2[3] = {V[2], V[5], V[8]};
    auto order = [](double &ea, double (&va)[3], double &eb, double (&vb)[3]) {
        if (eb > ea) {
            const double t = ea;
            ea = eb;
            eb = t;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double u = va[k];
                va[k] = vb[k];
                vb[k] = u;
            }
        }
    };
    order(e0, a0, e1, a1);
    order(e1, a1, e2, a2);
    order(e0, a0, e1, a1);
    if (!(e0 > 0.0)) {
        a0[0] = 1.0, a0[1] = 0.0, a0[2] = 0.0;
        a1[0] = 0.0, a1[1] = 1.0, a1[2] = 0.0;
    }
    // major and middle: the component of largest magnitude (of the returned floats, the lowest index on ties) positive
    auto fix_sign = [](double (&v)[3]) {
        const float f[3] = {(float) v[0], (float) v[1], (float) v[2]};
        int k = 0;
        if (fabsf(f[1]) > fabsf(f[0])) k = 1;
        if (fabsf(f[2]) > fabsf(f[k])) k = 2;
        if (f[k] < 0.f) {
            v[0] = -v[0];
            v[1] = -v[1];
            v[2] = -v[2];
        }
    };
    fix_sign(a0);
    fix_sign(a1);
    a2[0] = a0[1] * a1[2] - a0[2] * a1[1];
    a2[1] = a0[2] * a1[0] - a0[0] * a1[2];
    a2[2] = a0[0] * a1[1] - a0[1] * a1[0];
    b.eigenvalues[0] = (float) e0;
    b.eigenvalues[1] = (float) e1;
    b.eigenvalues[2] = (float) e2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.axes[k] = (float) a0[k];
        b.axes[3 + k] = (float) a1[k];
        b.axes[6 + k] = (float) a2[k];
    }
}

// PCL's computeOBB from the projections' extremes
__global__ void __launch_bounds__(kBlock)
    k_box_obb(const u64 *__restrict__ acc, unsigned n_clusters, wm_cluster_box *__restrict__ boxes,
              const unsigned *__restrict__ err) {
    const unsigned c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_clusters || err[0] != 0u) return;
    wm_cluster_box &b = boxes[c];
    if (b.n == 0u || (b.flags & WM_BOX_RANGE)) return;
    double mid[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = box_unkey(acc[(size_t) c * PassObb::W + k]), hi = box_unkey(acc[(size_t) c * PassObb::W + 3 + k]);
        b.obb_half[k] = (float) ((hi - lo) / 2.0);
        mid[k] = (hi + lo) / 2.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        b.obb_center[i] = (float) ((((double) b.centroid[i] + mid[0] * (double) b.axes[i]) + mid[1] * (double) b.axes[3 + i]) +
                                   mid[2] * (double) b.axes[6 + i]);
}

unsigned blocks_of(size_t n) { return (unsigned) ((n + kBlock - 1) / kBlock); }

bool mem_ok(int mem) { return mem == WM_MEM_HOST || mem == WM_MEM_DEVICE; }

}  // namespace

// The context's workspace of the cluster boxes: its own buffers, shared with nothing else on the context.
struct BoxesWs {
    DevBuf pts, idx, off;    // host inputs on their way
    DevBuf acc, sums, err;   // 8 words per cluster (the AABB pass, then the OBB pass), 27 (the sums), the two counters
    DevBuf tile_c;           // per tile of the member list: the cluster of its first member
    DevBuf boxes;            // a host output on its way
    PinnedBuf h_err;
};

void boxes_release(wm_ctx *ctx) {
    BoxesWs *w = static_cast<BoxesWs *>(ctx->boxes);
    if (!w) return;
    DevBuf *bufs[] = {&w->pts, &w->idx, &w->off, &w->acc, &w->sums, &w->err, &w->tile_c, &w->boxes};
    for (DevBuf *b : bufs) b->release();
    w->h_err.release();
    delete w;
    ctx->boxes = nullptr;
}

}  // namespace wm

using namespace wm;

extern "C" {

int wm_cluster_boxes(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const int32_t *indices, size_t n_members,
                     const uint32_t *offsets, size_t n_clusters, int list_mem, wm_cluster_box *boxes_out, int out_mem,
                     float *kernel_ms) {
    if (!ctx || (n_clusters > 0 && (!offsets || !boxes_out)) || stride < 12 || (stride & 3) || stride > 0xFFFFFFFCu ||
        !mem_ok(mem) || !mem_ok(list_mem) || !mem_ok(out_mem) || n > 0x7FFFFFF0u || n_members > 0x7FFFFFF0u ||
        n_clusters > 0x7FFFFFF0u || (n > 0 && !pts) || (!indices && n_members != n))
        return WM_ERR_ARG;
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_clusters == 0) return WM_OK;  // (no device is touched)

    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->boxes) ctx->boxes = new BoxesWs();
    BoxesWs &w = *static_cast<BoxesWs *>(ctx->boxes);
    hipStream_t st = ctx->stream;
    const unsigned nc = (unsigned) n_clusters;
    WM_HIP(ctx, w.acc.reserve((size_t) nc * PassAabb::W * sizeof(u64)));
    WM_HIP(ctx, w.sums.reserve((size_t) nc * PassSums::W * sizeof(u64)));
    WM_HIP(ctx, w.err.reserve(16));
    WM_HIP(ctx, w.h_err.reserve(16));
    if (kernel_ms) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));

    BoxList L{};
    L.pts = static_cast<const unsigned char *>(pts);
    L.n = (unsigned) n;
    L.stride = (unsigned) stride;
    L.indices = indices;
    L.n_members = (unsigned) n_members;
    L.offsets = offsets;
    L.n_clusters = nc;
    if (mem == WM_MEM_HOST && n > 0) {
        WM_HIP(ctx, w.pts.reserve(n * stride));
        WM_HIP(ctx, hipMemcpyAsync(w.pts.p, pts, n * stride, hipMemcpyHostToDevice, st));
        L.pts = w.pts.as<unsigned char>();
    }
    if (list_mem == WM_MEM_HOST) {
        if (indices && n_members > 0) {
            WM_HIP(ctx, w.idx.reserve(n_members * 4));
            WM_HIP(ctx, hipMemcpyAsync(w.idx.p, indices, n_members * 4, hipMemcpyHostToDevice, st));
            L.indices = w.idx.as<int>();
        }
        WM_HIP(ctx, w.off.reserve(((size_t) nc + 1) * 4));
        WM_HIP(ctx, hipMemcpyAsync(w.off.p, offsets, ((size_t) nc + 1) * 4, hipMemcpyHostToDevice, st));
        L.offsets = w.off.as<unsigned>();
    }
    wm_cluster_box *d_boxes = boxes_out;
    if (out_mem == WM_MEM_HOST) {
        WM_HIP(ctx, w.boxes.reserve((size_t) nc * sizeof(wm_cluster_box)));
        d_boxes = w.boxes.as<wm_cluster_box>();
    }
    u64 *acc = w.acc.as<u64>(), *sums = w.sums.as<u64>();
    unsigned *err = w.err.as<unsigned>();
    WM_HIP(ctx, hipMemsetAsync(err, 0, 16, st));
    WM_HIP(ctx, hipMemsetAsync(sums, 0, (size_t) nc * PassSums::W * sizeof(u64), st));

    const unsigned tiles = (unsigned) ((n_members + kBoxTile - 1) / kBoxTile), cblocks = blocks_of((size_t) nc + 1);
    WM_HIP(ctx, w.tile_c.reserve(((size_t) tiles + 1) * 4));
    unsigned *tile_c = w.tile_c.as<unsigned>();
    hipLaunchKernelGGL(k_box_check, dim3(cblocks), dim3(kBlock), 0, st, L.offsets, nc, L.n_members, acc, tile_c, tiles, err);
    if (tiles) hipLaunchKernelGGL(k_box_pass<PassAabb>, dim3(tiles), dim3(kBlock), 0, st, L, (const unsigned *) tile_c, tiles,
                                  (const wm_cluster_box *) d_boxes, acc, err);
    hipLaunchKernelGGL(k_box_mid, dim3(cblocks), dim3(kBlock), 0, st, (const u64 *) acc, nc, d_boxes, (const unsigned *) err);
    if (tiles) hipLaunchKernelGGL(k_box_pass<PassSums>, dim3(tiles), dim3(kBlock), 0, st, L, (const unsigned *) tile_c, tiles,
                                  (const wm_cluster_box *) d_boxes, sums, err);
    hipLaunchKernelGGL(k_box_eig, dim3(cblocks), dim3(kBlock), 0, st, (const u64 *) sums, nc, d_boxes, acc, (const unsigned *) err);
    if (tiles) hipLaunchKernelGGL(k_box_pass<PassObb>, dim3(tiles), dim3(kBlock), 0, st, L, (const unsigned *) tile_c, tiles,
                                  (const wm_cluster_box *) d_boxes, acc, err);
    hipLaunchKernelGGL(k_box_obb, dim3(cblocks), dim3(kBlock), 0, st, (const u64 *) acc, nc, d_boxes, (const unsigned *) err);
    WM_HIP(ctx, hipGetLastError());
    if (kernel_ms) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    // the one fetch: the two error counters (the stream has run to its end when they are here)
    unsigned *h_err = w.h_err.as<unsigned>();
    WM_TRY(fast_fetch(ctx, h_err, err, 8));
    if (kernel_ms) {
        WM_HIP(ctx, hipEventSynchronize(ctx->ev_b));
        (void) hipEventElapsedTime(kernel_ms, ctx->ev_a, ctx->ev_b);
    }
    if (h_err[0] != 0u || h_err[1] != 0u) return WM_ERR_ARG;
    if (out_mem == WM_MEM_HOST) WM_TRY(copy_to_caller(ctx, boxes_out, d_boxes, (size_t) nc * sizeof(wm_cluster_box)));
    return WM_OK;
}

}  // extern "C"
