// wm_ground.hip -- wave::GroundSegmentation<PointT>::applyFilter on device: libwave's Gaussian-process ground filter
// (Chen et al. 2014), wave_matching/include/wave/matching/impl/ground_segmentation.hpp:10-381.
//
// One call = S scans (wm_ground_segment: one; wm_ground_segment_batch: a queue of them) in a few launches on the
// context's stream and one host wait, for the counts (a second one only when the factors' block has to grow, see
// k_gs_sector).  Cells, sectors and slots are numbered scan after scan (scan k's cell c is k C + c), a point's index
// is local to its scan everywhere, and the scans' points lie one scan after the other in keys / vals / labels:
//   k_gs_bin       one thread per point: in range, sector, linear bin (impl :36-84); per-cell point count and the
//                  prototype (lowest z, first index) by one 64-bit atomicMin on (orderable z << 32 | index);
//                  sort key = scan (C + 1) + cell, the extra key per scan for the points out of range
//   sort           (key, index) pairs, stable (wm_sort.hpp's rs_sort_pairs): every cell's points in ascending index
//   scan           cell counts -> each cell's first place in the sorted pairs (less the out-of-range points of the
//                  scans before it, which the scan's offset restores)
//   k_gs_sector    one workgroup per sector of a scan (impl :108-355): signal cells (> 5 points), sorted by (height, bin),
//                  seeds, INSAC passes on a Cholesky factor of C_XX + p_sn I that grows by appended rows; per cell
//                  its kind (model / remaining / none), its rank within the sector and its reference height
//   k_gs_cells<1>  one wave per cell: labels, and per (list, sector, rank) the number of points of each list
//   scan           those counts (lists not kept count zero) -> every cell's first place in the output
//   k_gs_cells<0>  one wave per cell: the indices to their places (within a cell in input index order) and, when
//                  asked, the points themselves
//   k_gs_finish    the counts -> the scans' stats blocks, which the host fetches together
// Everything a decision rests on is formed in a fixed order inside one lane or one workgroup; the only atomics are
// integer ones (counts, the prototype minimum, the stats), so a call is bit-reproducible.
//
// Arithmetic, as the reference's text has it (tests/ground_reference.py gives the line for each):
//   in range  sqrt((double) (float) ((x*x + y*y) + z*z)) < rmax            (unqualified sqrt: C's double sqrt)
//   sector    (unsigned) (wrapTo360(atan2((double) y, (double) x) * (180 / M_PI)) / (360.0 / num_bins_a))
//   bin       (unsigned) ((double) sqrtf(x*x + y*y) / ((double) rmax / num_bins_l))   (sqrtf correctly rounded)
//   GP        double, kernel p_sf * exp(coeff * d^2) with float coeff = -1 / (2 p_l^2); inlier iff
//             vf < p_tmodel && |(h - f) / sqrt(p_sn + vf * vf)| < p_tdata against the pass-start model
//   labels    float h = |ref - z|: model cells h < p_tg ground, else h > robot_height overhanging, else obstacle;
//             remaining cells (sufficient model only) h > robot_height overhanging, else obstacle
// Where the reference is undefined: height ties go by ascending bin; a bin index that rounds up to
// num_bins_a / num_bins_l is clamped to the last bin; every call starts afresh; -0.0 ties with +0.0.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "wm_internal.hpp"
#include "wm_sort.hpp"
#include "wm_stage.hpp"

namespace wm {

namespace {

constexpr int kGsThreads = 256;
constexpr int kGsStatsLen = 16;  // u64: [0..2] list sizes, [3] in range, [4] signal cells, [5] model cells,
                                 // [6] sufficient sectors, [7] passes, [8] max passes, [9] output size; a block per
                                 // scan, and behind the last one the call's [0] overflow, [1] bump counter
constexpr int kGsTailLen = 2;
enum { kKindNone = 0, kKindModel = 1, kKindRest = 2 };

struct GsParams {
    double rmax, bsize_rad, bsize_lin, robot_height, max_seed_range, max_seed_height;
    double p_sf, p_sn, p_tmodel, p_tdata, coeff;  // the float parameters' values, in double
    float p_tg;
    int num_seed_points, A, L;
    unsigned C;  // A * L
};

struct GsScan {  // one scan of a call
    const unsigned char *raw;
    unsigned n;     // points
    unsigned off;   // its first place among the call's points
    unsigned blk0;  // its first workgroup of k_gs_bin (a workgroup's points are of one scan)
    unsigned pad;
};

struct GsScans {  // the scans of a call: a table in device memory, or (tab == nullptr) the one scan `one`
    const GsScan *tab;
    GsScan one;
    unsigned S;
};

struct GsCell {
    double ref;  // model cells: the model height (the prototype's z); remaining cells: the last pass's prediction
    int rank;    // place of the cell within its sector's output (model order, then the remaining cells); -1: none
    int kind;
};

struct GsSector {  // the per-sector slices (num_bins_l entries each) of the sector kernel's scratch
    double *sig_r, *sig_h, *srt_r, *srt_h, *fpred, *su;
    int *sig_b, *srt_b, *model, *rest, *inl;
};

// float -> unsigned whose unsigned order is the float order (-0.0 canonicalised to +0.0 first)
__device__ __forceinline__ unsigned gs_orderable(float z) {
    const unsigned b = __float_as_uint(z == 0.f ? 0.f : z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ const float *gs_point(const unsigned char *raw, size_t stride, unsigned i) {
    return reinterpret_cast<const float *>(raw + (size_t) i * stride);
}

__device__ __forceinline__ GsScan gs_scan(const GsScans &sc, unsigned k) {
    if (!sc.tab) return sc.one;
    return sc.tab[k];
}

// (sqrtf: correctly rounded, as std::sqrt(float) is on the host; HIP's __fsqrt_rn is the native approximation)
__device__ __forceinline__ float gs_xy(float x, float y) {
    return sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
}

// impl :48-80
__global__ void __launch_bounds__(kBlock)
    k_gs_bin(GsScans sc, size_t stride, GsParams p, unsigned *__restrict__ keys, unsigned *__restrict__ vals,
             unsigned *__restrict__ counts, unsigned long long *__restrict__ proto) {
    unsigned k = 0;
    if (sc.tab) {  // the last scan that starts at or before this workgroup (empty scans take no workgroup)
        unsigned hi = sc.S;
        while (hi - k > 1u) {
            const unsigned mid = (k + hi) >> 1;
            if (sc.tab[mid].blk0 <= blockIdx.x) k = mid;
            else hi = mid;
        }
    }
    const GsScan me = gs_scan(sc, k);
    const unsigned i = (blockIdx.x - me.blk0) * kBlock + threadIdx.x;
    if (i >= me.n) return;
    const float *q = gs_point(me.raw, stride, i);
    const float x = q[0], y = q[1], z = q[2];
    const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
    unsigned key = k * (p.C + 1u) + p.C;  // out of range (NaN / inf included): sorts behind every cell of the scan
    if (sqrt((double) r2) < p.rmax) {
        double ph = atan2((double) y, (double) x) * (180.0 / M_PI);
        ph = ph > 0 ? fmod(ph, 360.0) : fmod(ph + 360.0, 360.0);  // wrapTo360, wave_utils/src/math.cpp:80-87
        unsigned br = (unsigned) (ph / p.bsize_rad);
        unsigned bl = (unsigned) ((double) gs_xy(x, y) / p.bsize_lin);
        if (br >= (unsigned) p.A) br = (unsigned) p.A - 1u;  // (b)
        if (bl >= (unsigned) p.L) bl = (unsigned) p.L - 1u;
        const unsigned cell = br * (unsigned) p.L + bl;
        key = k * (p.C + 1u) + cell;
        atomicAdd(&counts[(size_t) k * p.C + cell], 1u);
        atomicMin(&proto[(size_t) k * p.C + cell], ((unsigned long long) gs_orderable(z) << 32) | i);
    }
    keys[me.off + i] = key;
    vals[me.off + i] = i;
}

__device__ __forceinline__ double gs_cov(const GsParams &p, double a, double b) {  // impl :96-101
    const double d = a - b;
    return p.p_sf * exp(p.coeff * (d * d));
}

__device__ __forceinline__ bool gs_before(double ha, int ba, double hb, int bb) {  // sort by height, then bin (a)
    return ha < hb || (ha == hb && ba < bb);
}

// One workgroup per sector of a scan: impl :108-355.  The sector's slices live in HBM (num_bins_l is a user parameter);
// the factor and the per-point solves in `mat`, a block of m * m + m (m + 1) / 2 doubles taken from the bump
// counter (m = the sector's signal cells).  A sector whose block does not fit flags it (stats[10]) and skips its
// passes; the host then grows `mat` to the bump counter's total and runs the sector kernel again.  `stats`: the
// scans' blocks; `tail`: the call's overflow count and bump counter.
__global__ void __launch_bounds__(kGsThreads)
    k_gs_sector(GsScans sc, size_t stride, GsParams p, const unsigned *__restrict__ counts,
                const unsigned long long *__restrict__ proto, GsSector ws, double *__restrict__ mat, size_t mat_cap,
                unsigned long long *__restrict__ tail, GsCell *__restrict__ cells, unsigned long long *__restrict__ stats) {
    __shared__ unsigned s_wave[kGsThreads / 64];
    __shared__ int s_q, s_r, s_go, s_base;
    __shared__ size_t s_off;
    const int tid = threadIdx.x, L = p.L;
    const unsigned scan = blockIdx.x / (unsigned) p.A;
    const unsigned char *raw = gs_scan(sc, scan).raw;
    stats += (size_t) scan * kGsStatsLen;
    const size_t sl = (size_t) blockIdx.x * L;  // (scan k's sector s: k A + s, its cells from (k A + s) L = k C + s L)
    double *sig_r = ws.sig_r + sl, *sig_h = ws.sig_h + sl, *srt_r = ws.srt_r + sl, *srt_h = ws.srt_h + sl;
    double *fpred = ws.fpred + sl, *su = ws.su + sl;
    int *sig_b = ws.sig_b + sl, *srt_b = ws.srt_b + sl, *model = ws.model + sl, *rest = ws.rest + sl, *inl = ws.inl + sl;
    GsCell *cell = cells + sl;

    // every cell of the sector: unlabelled until said otherwise
    for (int j = tid; j < L; j += kGsThreads) cell[j] = GsCell{0.0, -1, kKindNone};
    // signal cells in ascending bin (impl :117-135): range = xy of the prototype, height = its z
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int j0 = 0; j0 < L; j0 += kGsThreads) {
        const int j = j0 + tid;
        const bool sig = j < L && counts[sl + j] > 5u;
        const unsigned ex = rs_block_exclusive(sig ? 1u : 0u, s_wave);
        const int base = s_base;
        if (sig) {
            const unsigned pi = (unsigned) (proto[sl + j] & 0xFFFFFFFFull);
            const float *q = gs_point(raw, stride, pi);
            sig_r[base + (int) ex] = (double) gs_xy(q[0], q[1]);
            sig_h[base + (int) ex] = (double) q[2];
            sig_b[base + (int) ex] = j;
        }
        __syncthreads();
        if (tid == kGsThreads - 1) s_base = base + (int) ex + (sig ? 1 : 0);
        __syncthreads();
    }
    const int m = s_base;
    if (m == 0) return;
    // sorted by (height, bin): a point's place = the number of points before it (the keys are distinct)
    for (int k = tid; k < m; k += kGsThreads) {
        const double h = sig_h[k];
        const int b = sig_b[k];
        int rank = 0;
        for (int t = 0; t < m; ++t) rank += gs_before(sig_h[t], sig_b[t], h, b) ? 1 : 0;
        srt_r[rank] = sig_r[k];
        srt_h[rank] = h;
        srt_b[rank] = b;
    }
    __syncthreads();
    // seeds (impl :143-186), one lane: the walk takes an eligible point before it checks the count
    if (tid == 0) {
        const size_t want = p.num_seed_points < 0 ? (size_t) m : min((size_t) m, (size_t) p.num_seed_points);
        int q = 0, r = 0, cur = 0;
        size_t taken = 0;
        while (cur < m) {
            if (srt_r[cur] < p.max_seed_range && fabs(srt_h[cur]) < p.max_seed_height) {
                model[q++] = cur;
                ++taken;
            } else {
                rest[r++] = cur;
            }
            ++cur;
            if (taken >= want) break;
        }
        for (; cur < m; ++cur) rest[r++] = cur;  // (the points after the walk stopped keep their order)
        s_q = q;
        s_r = r;
        s_go = (q >= 2 && r > 0) ? 1 : 0;
        s_off = 0;
        if (s_go) {
            const size_t need = (size_t) m * m + (size_t) m * (m + 1) / 2;
            const size_t off = (size_t) atomicAdd(&tail[1], (unsigned long long) need);
            if (off + need <= mat_cap) {
                s_off = off;
            } else {  // (`mat` too small: flagged, nothing written; the host grows it and runs this kernel again)
                s_go = 0;
                atomicAdd(&tail[0], 1ull);
            }
        }
    }
    __syncthreads();
    const bool sufficient = s_q >= 2;
    double *Lm = mat + s_off;                      // packed lower triangle: row i at i (i + 1) / 2
    double *W = Lm + (size_t) m * (m + 1) / 2;     // W[c * m + i]: L^-1 c_i of remaining point i
    int q_old = 0, passes = 0;
    while (s_go) {  // impl :202-286
        ++passes;
        const int q = s_q, r = s_r;
        // new rows of C_XX + p_sn I and of z (the factor and L^-1 z are extended, never refactored: row k of a
        // Cholesky factor depends on rows < k only, so this is the factor of the whole model, bit for bit)
        for (int row = q_old; row < q; ++row) {
            double *Lr = Lm + (size_t) row * (row + 1) / 2;
            const double xr = srt_r[model[row]];
            for (int c = tid; c <= row; c += kGsThreads) Lr[c] = gs_cov(p, xr, srt_r[model[c]]) + (c == row ? p.p_sn : 0.0);
        }
        for (int row = q_old + tid; row < q; row += kGsThreads) su[row] = srt_h[model[row]];
        __syncthreads();
        // right-looking over the columns, new rows only: entry (r, c) is K_rc - l_r0 l_c0 - l_r1 l_c1 - ... in
        // ascending order, then / l_cc (sqrt on the diagonal) -- the sequential formula's order
        for (int c = 0; c < q; ++c) {
            double *Lc = Lm + (size_t) c * (c + 1) / 2;
            if (c >= q_old && tid == 0) {
                const double d = sqrt(Lc[c]);
                Lc[c] = d;
                su[c] = su[c] / d;
            }
            __syncthreads();
            const int r0 = max(c + 1, q_old);
            for (int row = r0 + tid; row < q; row += kGsThreads) {
                double *Lr = Lm + (size_t) row * (row + 1) / 2;
                Lr[c] = Lr[c] / Lc[c];
            }
            __syncthreads();
            const int w = q - c - 1;
            if (w > 0 && r0 < q) {
                const long long nr = q - r0;
                for (long long idx = tid; idx < nr * w; idx += kGsThreads) {
                    const int row = r0 + (int) (idx / w), cp = c + 1 + (int) (idx % w);
                    if (cp > row) continue;
                    double *Lr = Lm + (size_t) row * (row + 1) / 2;
                    const double *Lp = Lm + (size_t) cp * (cp + 1) / 2;
                    Lr[cp] = Lr[cp] - Lr[c] * Lp[c];
                }
                for (int cp = r0 + tid; cp < q; cp += kGsThreads) {
                    const double *Lp = Lm + (size_t) cp * (cp + 1) / 2;
                    su[cp] = su[cp] - Lp[c] * su[c];
                }
            }
            __syncthreads();
        }
        // every remaining point against the pass-start model: w = L^-1 c_i, f = w . u, vf = p_sf - w . w
        for (int i = tid; i < r; i += kGsThreads) {
            const double xi = srt_r[rest[i]];
            double acc_f = 0.0, acc_v = 0.0;
            for (int c = 0; c < q; ++c) {
                const double *Lc = Lm + (size_t) c * (c + 1) / 2;
                double sacc = gs_cov(p, xi, srt_r[model[c]]);
                for (int t = 0; t < c; ++t) sacc = sacc - Lc[t] * W[(size_t) t * m + i];
                const double wc = sacc / Lc[c];
                W[(size_t) c * m + i] = wc;
                acc_f = acc_f + wc * su[c];
                acc_v = acc_v + wc * wc;
            }
            const double vf = p.p_sf - acc_v;
            const double met = (srt_h[rest[i]] - acc_f) / sqrt(p.p_sn + vf * vf);
            fpred[i] = acc_f;
            inl[i] = (vf < p.p_tmodel && fabs(met) < p.p_tdata) ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0) {  // inliers to the end of the model in their order; the rest keep theirs (and their prediction)
            int qq = q, j = 0;
            for (int i = 0; i < r; ++i) {
                if (inl[i]) {
                    model[qq++] = rest[i];
                } else {
                    rest[j] = rest[i];
                    fpred[j] = fpred[i];
                    ++j;
                }
            }
            s_q = qq;
            s_r = j;
            s_go = (qq != q && j > 0) ? 1 : 0;
        }
        q_old = q;
        __syncthreads();
    }
    // per cell: kind, rank within the sector, reference height (impl :293-354)
    const int q = s_q, r = s_r;
    for (int k = tid; k < q; k += kGsThreads) cell[srt_b[model[k]]] = GsCell{srt_h[model[k]], k, kKindModel};
    if (sufficient)
        for (int i = tid; i < r; i += kGsThreads) cell[srt_b[rest[i]]] = GsCell{fpred[i], q + i, kKindRest};
    if (tid == 0) {
        atomicAdd(&stats[4], (unsigned long long) m);
        atomicAdd(&stats[5], (unsigned long long) q);
        if (sufficient) atomicAdd(&stats[6], 1ull);
        atomicAdd(&stats[7], (unsigned long long) passes);
        atomicMax(&stats[8], (unsigned long long) passes);
    }
}

__device__ __forceinline__ int gs_label(const GsParams &p, const GsCell &c, float z) {  // impl :302-319, :336-348
    const float h = (float) fabs(c.ref - (double) z);
    if (c.kind == kKindModel && h < p.p_tg) return WM_GROUND_GROUND;
    return (double) h > p.robot_height ? WM_GROUND_OVERHANGING : WM_GROUND_OBSTACLE;
}

// One wave per cell: its points (ascending index) are labelled 64 at a time.  COUNT: the per-(scan, list, sector,
// rank) counts (a list that is not kept counts zero) and the lists' sizes; else the indices (and, with `pout`, the
// points' x y z in records of out_stride bytes, the rest zero) go to their places.
template <bool COUNT>
__global__ void __launch_bounds__(kBlock)
    k_gs_cells(GsScans sc, size_t stride, GsParams p, const GsCell *__restrict__ cells,
               const unsigned *__restrict__ cell_start, const unsigned *__restrict__ sorted_idx, int keep,
               unsigned *__restrict__ slot, unsigned long long *__restrict__ stats, unsigned char *__restrict__ labels,
               int *__restrict__ out, size_t cap, unsigned char *__restrict__ pout, size_t out_stride) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (c >= sc.S * p.C) return;
    const GsCell ci = cells[c];
    if (ci.rank < 0) return;
    const unsigned scan = c / p.C;
    const GsScan me = gs_scan(sc, scan);
    const unsigned char *raw = me.raw;
    // slots: scan-major, within a scan list-major, within a list by (sector, rank): scan k's list l from (3 k + l) C
    const size_t sidx = (size_t) (c / (unsigned) p.L) * p.L + (size_t) ci.rank + (size_t) 2 * scan * p.C;
    // the scan's points lie at [me.off, me.off + me.n) of the sorted pairs, its cells first
    const unsigned shift = me.off - cell_start[(size_t) scan * p.C];
    const unsigned beg = cell_start[c] + shift, end = cell_start[c + 1] + shift;
    unsigned run[3] = {0u, 0u, 0u};
    if (!COUNT)
        for (int l = 0; l < 3; ++l) run[l] = slot[(size_t) l * p.C + sidx];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (unsigned b = beg; b < end; b += 64u) {
        const unsigned pos = b + lane;
        const bool live = pos < end;
        unsigned pi = 0u;
        int lab = 0;
        if (live) {
            pi = sorted_idx[pos];
            lab = gs_label(p, ci, gs_point(raw, stride, pi)[2]);
            if (COUNT && labels) labels[(size_t) me.off + pi] = (unsigned char) lab;
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const unsigned long long mk = __ballot(live && lab == l + 1);
            if (!COUNT && live && lab == l + 1 && (keep >> l) & 1) {
                const size_t o = (size_t) run[l] + (size_t) __popcll(mk & lt);
                if (o < cap) {
                    out[o] = (int) pi;
                    if (pout) {
                        const unsigned *q = reinterpret_cast<const unsigned *>(gs_point(raw, stride, pi));
                        unsigned *w = reinterpret_cast<unsigned *>(pout + o * out_stride);
                        w[0] = q[0], w[1] = q[1], w[2] = q[2];
                        for (size_t j = 3; j < out_stride / 4; ++j) w[j] = 0u;
                    }
                }
            }
            run[l] += (unsigned) __popcll(mk);
        }
    }
    if (COUNT && lane == 0) {
        for (int l = 0; l < 3; ++l) {
            slot[(size_t) l * p.C + sidx] = ((keep >> l) & 1) ? run[l] : 0u;
            if (run[l]) atomicAdd(&stats[(size_t) scan * kGsStatsLen + l], (unsigned long long) run[l]);
        }
    }
}

__global__ void k_gs_finish(const unsigned *__restrict__ cell_start, const unsigned *__restrict__ slot_base, unsigned C,
                            unsigned S, unsigned long long *__restrict__ stats) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < S) {
        stats[(size_t) k * kGsStatsLen + 3] = cell_start[(size_t) (k + 1) * C] - cell_start[(size_t) k * C];
        stats[(size_t) k * kGsStatsLen + 9] = slot_base[3ull * (k + 1) * C] - slot_base[3ull * k * C];
    }
}

}  // namespace

// The context's workspace of this filter: its own buffers, shared with nothing else on the context.
struct GroundWs {
    DevBuf raw, keys, vals, keys2, vals2, sort_tmp, counts, proto, cell_start, cells, slot, slot_base, sector, mat,
        stats, labels, out, pts;
    PairStage stage;                        // a batch's scan table and host clouds up, its stats back (wm_stage.hpp)
    unsigned long long *h_stats = nullptr;  // pinned: the single call's stats block and tail
    size_t mat_need = 0;                    // doubles the sectors' factor blocks took in the last call
};

void ground_release(wm_ctx *ctx) {
    GroundWs *g = static_cast<GroundWs *>(ctx->ground);
    if (!g) return;
    DevBuf *bufs[] = {&g->raw, &g->keys, &g->vals, &g->keys2, &g->vals2, &g->sort_tmp, &g->counts, &g->proto,
                      &g->cell_start, &g->cells, &g->slot, &g->slot_base, &g->sector, &g->mat, &g->stats,
                      &g->labels, &g->out, &g->pts};
    for (DevBuf *b : bufs) b->release();
    g->stage.release();
    if (g->h_stats) (void) hipHostFree(g->h_stats);
    delete g;
    ctx->ground = nullptr;
}

namespace {

// One call's launches, for wm_ground_segment (a scan handed over by value) and wm_ground_segment_batch (a table).
struct GsCall {
    GsScans sc;
    GsParams p;
    size_t stride = 0, total = 0;  // the scans' points in all
    unsigned bin_blocks = 0;
    int keep = 0;
    unsigned char *labels = nullptr;  // total entries, or nullptr
    int *out = nullptr;
    size_t out_cap = 0;
    unsigned char *pout = nullptr;
    size_t out_stride = 0;
    unsigned long long *dstats = nullptr;  // S blocks and the tail
    GsSector ws;
    size_t cells() const { return (size_t) sc.S * p.C; }
    size_t stats_len() const { return (size_t) sc.S * kGsStatsLen + kGsTailLen; }
};

void gs_fill_params(const wm_ground_params *params, unsigned C, GsParams &p) {
    p.rmax = params->rmax;
    p.bsize_rad = 360.0 / params->num_bins_a;                 // impl :39
    p.bsize_lin = params->rmax / params->num_bins_l;          // impl :40
    p.robot_height = params->robot_height;
    p.max_seed_range = params->max_seed_range;
    p.max_seed_height = params->max_seed_height;
    p.p_sf = params->p_sf;
    p.p_sn = params->p_sn;
    p.p_tmodel = params->p_tmodel;
    p.p_tdata = params->p_tdata;
    p.coeff = (float) (-1 / (2 * params->p_l * params->p_l));  // impl :96 (float)
    p.p_tg = params->p_tg;
    p.num_seed_points = params->num_seed_points;
    p.A = params->num_bins_a;
    p.L = params->num_bins_l;
    p.C = C;
}

// the buffers of S scans of C cells and `total` points
int gs_reserve(wm_ctx *ctx, GroundWs &g, GsCall &c, const char *who) {
    const size_t nb = c.total ? c.total : 1, SC = c.cells();
    WM_HIP(ctx, g.keys.reserve(nb * 4));
    WM_HIP(ctx, g.vals.reserve(nb * 4));
    WM_HIP(ctx, g.keys2.reserve(nb * 4));
    WM_HIP(ctx, g.vals2.reserve(nb * 4));
    WM_HIP(ctx, g.counts.reserve(SC * 4));
    WM_HIP(ctx, g.proto.reserve(SC * 8));
    WM_HIP(ctx, g.cell_start.reserve((SC + 1) * 4));
    WM_HIP(ctx, g.cells.reserve(SC * sizeof(GsCell)));
    WM_HIP(ctx, g.slot.reserve(3 * SC * 4));
    WM_HIP(ctx, g.slot_base.reserve((3 * SC + 1) * 4));
    WM_HIP(ctx, g.sector.reserve(SC * (6 * sizeof(double) + 5 * sizeof(int))));
    // the sectors' factor blocks (m * m + m (m + 1) / 2 doubles for m signal cells) are taken from `mat` on the device;
    // it starts at the last call's need (8 MiB at least: the fixture takes 0.5, a 1M-point ring scan 5.2) and, when a
    // sector finds it too small, grows to what the sectors of all scans asked for in all, and the sector kernel and
    // what follows it run again
    if (g.mat.reserve(std::max<size_t>(g.mat_need, (size_t) 1 << 20) * sizeof(double)) != hipSuccess) {
        (void) hipGetLastError();
        ctx->last_error = std::string(who) + ": factor workspace";
        return WM_ERR_NOMEM;
    }
    if (c.total) WM_HIP(ctx, g.sort_tmp.reserve(rs_temp_bytes(c.total)));
    unsigned char *b = g.sector.as<unsigned char>();
    double **d[] = {&c.ws.sig_r, &c.ws.sig_h, &c.ws.srt_r, &c.ws.srt_h, &c.ws.fpred, &c.ws.su};
    for (double **x : d) {
        *x = reinterpret_cast<double *>(b);
        b += SC * sizeof(double);
    }
    int **iv[] = {&c.ws.sig_b, &c.ws.srt_b, &c.ws.model, &c.ws.rest, &c.ws.inl};
    for (int **x : iv) {
        *x = reinterpret_cast<int *>(b);
        b += SC * sizeof(int);
    }
    return WM_OK;
}

// bins, the sort, the cells' places
int gs_front(wm_ctx *ctx, GroundWs &g, const GsCall &c) {
    hipStream_t st = ctx->stream;
    const size_t SC = c.cells();
    if (c.labels && c.total) WM_HIP(ctx, hipMemsetAsync(c.labels, 0, c.total, st));  // WM_GROUND_NONE
    WM_HIP(ctx, hipMemsetAsync(g.counts.p, 0, SC * 4, st));
    WM_HIP(ctx, hipMemsetAsync(g.proto.p, 0xFF, SC * 8, st));
    if (c.total) {
        unsigned *keys = g.keys.as<unsigned>(), *vals = g.vals.as<unsigned>();
        hipLaunchKernelGGL(k_gs_bin, dim3(c.bin_blocks), dim3(kBlock), 0, st, c.sc, c.stride, c.p, keys, vals,
                           g.counts.as<unsigned>(), g.proto.as<unsigned long long>());
        WM_HIP(ctx, hipGetLastError());
        const unsigned long long top = (unsigned long long) c.sc.S * (c.p.C + 1ull) - 1ull;  // the largest key
        unsigned bits = 1;
        while (bits < 32 && (top >> bits) != 0ull) ++bits;
        WM_HIP(ctx, rs_sort_pairs(g.sort_tmp.p, keys, g.keys2.as<unsigned>(), vals, g.vals2.as<unsigned>(), c.total, bits, st));
    }
    return exclusive_scan(ctx, g.counts.as<unsigned>(), SC, g.cell_start.as<unsigned>());
}

// sectors, labels, places, indices, stats (again from here when the factor workspace had to grow)
int gs_back(wm_ctx *ctx, GroundWs &g, const GsCall &c, int attempt) {
    hipStream_t st = ctx->stream;
    const size_t SC = c.cells();
    const unsigned cell_blocks = (unsigned) ((SC + kBlock / 64 - 1) / (kBlock / 64));
    const unsigned *vals2 = g.vals2.as<unsigned>();
    GsCell *cells = g.cells.as<GsCell>();
    WM_HIP(ctx, hipMemsetAsync(c.dstats, 0, c.stats_len() * sizeof(unsigned long long), st));
    WM_HIP(ctx, hipMemsetAsync(g.slot.p, 0, 3 * SC * 4, st));
    if (c.labels && c.total && attempt) WM_HIP(ctx, hipMemsetAsync(c.labels, 0, c.total, st));
    hipLaunchKernelGGL(k_gs_sector, dim3(c.sc.S * (unsigned) c.p.A), dim3(kGsThreads), 0, st, c.sc, c.stride, c.p,
                       (const unsigned *) g.counts.p, (const unsigned long long *) g.proto.p, c.ws, g.mat.as<double>(),
                       g.mat.cap / sizeof(double), c.dstats + (size_t) c.sc.S * kGsStatsLen, cells, c.dstats);
    WM_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gs_cells<true>), dim3(cell_blocks), dim3(kBlock), 0, st, c.sc, c.stride, c.p,
                       (const GsCell *) cells, (const unsigned *) g.cell_start.p, vals2, c.keep, g.slot.as<unsigned>(),
                       c.dstats, c.labels, (int *) nullptr, (size_t) 0, (unsigned char *) nullptr, (size_t) 0);
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(exclusive_scan(ctx, g.slot.as<unsigned>(), 3 * SC, g.slot_base.as<unsigned>()));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gs_cells<false>), dim3(cell_blocks), dim3(kBlock), 0, st, c.sc, c.stride, c.p,
                       (const GsCell *) cells, (const unsigned *) g.cell_start.p, vals2, c.keep,
                       g.slot_base.as<unsigned>(), c.dstats, (unsigned char *) nullptr, c.out, c.out_cap, c.pout,
                       c.out_stride);
    hipLaunchKernelGGL(k_gs_finish, dim3((c.sc.S + 63u) / 64u), dim3(64), 0, st, (const unsigned *) g.cell_start.p,
                       (const unsigned *) g.slot_base.p, c.p.C, c.sc.S, c.dstats);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

void gs_stats_out(const unsigned long long *hs, wm_ground_stats *stats) {
    stats->n_ground = (size_t) hs[0];
    stats->n_obstacle = (size_t) hs[1];
    stats->n_overhanging = (size_t) hs[2];
    stats->n_in_range = (size_t) hs[3];
    stats->n_signal_cells = (int) hs[4];
    stats->n_model_cells = (int) hs[5];
    stats->n_sufficient_sectors = (int) hs[6];
    stats->passes_total = (int) hs[7];
    stats->passes_max = (int) hs[8];
}

}  // namespace

}  // namespace wm

using namespace wm;

static bool gs_params_ok(const wm_ground_params *p) {
    const float f[] = {p->p_l, p->p_sf, p->p_sn, p->p_tmodel, p->p_tdata, p->p_tg};
    const double d[] = {p->rmax, p->robot_height, p->max_seed_range, p->max_seed_height};
    for (float v : f)
        if (!std::isfinite(v)) return false;
    for (double v : d)
        if (!std::isfinite(v)) return false;
    return p->num_bins_a > 0 && p->num_bins_l > 0 && p->p_l > 0.f && p->p_sf > 0.f && p->p_sn > 0.f;
}

extern "C" void wm_ground_default_params(wm_ground_params *p) {
    if (!p) return;
    p->rmax = 100;
    p->max_bin_points = 200;
    p->num_seed_points = 10;
    p->p_l = 4;
    p->p_sf = 1;
    p->p_sn = 0.3f;
    p->p_tmodel = 5;
    p->p_tdata = 5;
    p->p_tg = 0.3f;
    p->robot_height = 1.2;
    p->max_seed_range = 50;
    p->max_seed_height = 15;
    p->num_bins_a = 72;
    p->num_bins_l = 200;
}

// One scan, handed to the kernels by value: no table, no staging, the cloud copied from where it is.  This is
// wm_ground_segment, and wm_ground_segment_batch for a batch of one (arguments checked by the callers).
static int gs_one(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_ground_params *params,
                  int keep_mask, int32_t *indices_out, size_t cap, void *points_out, size_t out_stride, int out_mem,
                  size_t *n_out, uint8_t *labels_out, wm_ground_stats *stats, float *kernel_ms) {
    const uint64_t C64 = (uint64_t) params->num_bins_a * (uint64_t) params->num_bins_l;
    if (C64 > (1ull << 24)) return WM_ERR_NOMEM;  // (a cell costs ~120 bytes of workspace)
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->ground) ctx->ground = new GroundWs();
    GroundWs &g = *static_cast<GroundWs *>(ctx->ground);
    constexpr size_t kLen = kGsStatsLen + kGsTailLen;
    if (!g.h_stats) WM_HIP(ctx, hipHostMalloc((void **) &g.h_stats, kLen * sizeof(unsigned long long), hipHostMallocDefault));
    hipStream_t st = ctx->stream;

    GsCall c;
    gs_fill_params(params, (unsigned) C64, c.p);
    c.sc = GsScans{nullptr, GsScan{static_cast<const unsigned char *>(pts), (unsigned) n, 0u, 0u, 0u}, 1u};
    c.stride = stride;
    c.total = n;
    c.bin_blocks = (unsigned) ((n + kBlock - 1) / kBlock);
    c.keep = keep_mask;
    WM_TRY(gs_reserve(ctx, g, c, "wm_ground_segment"));
    WM_HIP(ctx, g.stats.reserve(kLen * sizeof(unsigned long long)));
    c.dstats = g.stats.as<unsigned long long>();
    if (mem == WM_MEM_HOST && n) {
        WM_HIP(ctx, g.raw.reserve(n * stride));
        WM_HIP(ctx, hipMemcpyAsync(g.raw.p, pts, n * stride, hipMemcpyHostToDevice, st));
        c.sc.one.raw = g.raw.as<unsigned char>();
    }
    if (labels_out && n) {
        if (out_mem == WM_MEM_DEVICE) {
            c.labels = labels_out;
        } else {
            WM_HIP(ctx, g.labels.reserve(n));
            c.labels = g.labels.as<unsigned char>();
        }
    }
    c.out = reinterpret_cast<int *>(indices_out);
    c.out_cap = cap;
    c.pout = static_cast<unsigned char *>(points_out);
    c.out_stride = points_out ? out_stride : 0;
    if (out_mem == WM_MEM_HOST) {
        WM_HIP(ctx, g.out.reserve((n ? n : 1) * 4));
        c.out = g.out.as<int>();
        c.out_cap = n;
        if (points_out) {  // (no more than n points can be kept)
            c.out_cap = std::min(cap, n);
            WM_HIP(ctx, g.pts.reserve((c.out_cap ? c.out_cap : 1) * out_stride));
            c.pout = g.pts.as<unsigned char>();
        }
    }
    if (kernel_ms) WM_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    WM_TRY(gs_front(ctx, g, c));
    const unsigned long long *hs = g.h_stats;
    for (int attempt = 0;; ++attempt) {
        WM_TRY(gs_back(ctx, g, c, attempt));
        if (kernel_ms) WM_HIP(ctx, hipEventRecord(ctx->ev_b, st));
        WM_HIP(ctx, hipMemcpyAsync(g.h_stats, c.dstats, kLen * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        WM_HIP(ctx, hipStreamSynchronize(st));      // the one wait (two when `mat` had to grow)
        g.mat_need = (size_t) hs[kGsStatsLen + 1];  // (the bump counter: every sector's request, granted or not)
        if (!hs[kGsStatsLen]) break;
        if (attempt || g.mat.reserve(g.mat_need * sizeof(double)) != hipSuccess) {
            (void) hipGetLastError();
            ctx->last_error = "wm_ground_segment: factor workspace";
            return WM_ERR_NOMEM;
        }
    }
    const size_t total = (size_t) hs[9];
    *n_out = total;
    if (stats) gs_stats_out(hs, stats);
    if (kernel_ms) (void) hipEventElapsedTime(kernel_ms, ctx->ev_a, ctx->ev_b);
    if (out_mem == WM_MEM_HOST) {
        const size_t m = std::min(total, cap);
        if (labels_out && n) WM_HIP(ctx, hipMemcpy(labels_out, c.labels, n, hipMemcpyDeviceToHost));
        if (m) WM_HIP(ctx, hipMemcpy(indices_out, c.out, m * 4, hipMemcpyDeviceToHost));
        if (m && points_out) WM_HIP(ctx, hipMemcpy(points_out, c.pout, m * out_stride, hipMemcpyDeviceToHost));
    }
    return total > cap ? WM_ERR_ARG : WM_OK;
}

extern "C" {

int wm_ground_segment(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, const wm_ground_params *params,
                      int keep_mask, int32_t *indices_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out,
                      wm_ground_stats *stats) {
    if (!ctx || !params || !n_out || (n > 0 && !pts) || stride < 12 || (stride & 3) || n > 0x7FFFFFF0u ||
        (cap > 0 && !indices_out) || keep_mask < 0 || keep_mask > 7 ||
        (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) || (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE) ||
        !gs_params_ok(params))
        return WM_ERR_ARG;
    *n_out = 0;
    if (stats) *stats = wm_ground_stats{};
    return gs_one(ctx, pts, n, stride, mem, params, keep_mask, indices_out, cap, nullptr, 0, out_mem, n_out, labels_out,
                  stats, nullptr);
}

int wm_ground_segment_batch(wm_ctx *ctx, const wm_ground_scan *scans, int n_scans, size_t stride, int mem,
                            const wm_ground_params *params, int keep_mask, int32_t *indices_out, size_t cap,
                            void *points_out, size_t out_stride, int out_mem, size_t *offsets_out, uint8_t *labels_out,
                            wm_ground_stats *stats, float *kernel_ms) {
    if (!ctx || n_scans < 0 || (n_scans > 0 && !scans) || !params || !offsets_out || stride < 12 || (stride & 3) ||
        (cap > 0 && !indices_out) || (points_out && (out_stride < 12 || (out_stride & 3))) || keep_mask < 0 ||
        keep_mask > 7 || (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) ||
        (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE) || !gs_params_ok(params))
        return WM_ERR_ARG;
    const unsigned S = (unsigned) n_scans;
    size_t total = 0, cloud_bytes = 0, blocks = 0;
    for (unsigned k = 0; k < S; ++k) {
        if ((scans[k].n > 0 && !scans[k].pts) || scans[k].n > WM_GROUND_BATCH_MAX_POINTS) return WM_ERR_ARG;
        total += scans[k].n;
        if (total > WM_GROUND_BATCH_MAX_POINTS) return WM_ERR_ARG;
        cloud_bytes += align_up256(scans[k].n * stride);
        blocks += (scans[k].n + kBlock - 1) / kBlock;
    }
    const uint64_t C64 = (uint64_t) params->num_bins_a * (uint64_t) params->num_bins_l;
    if ((uint64_t) S * (C64 + 1) > WM_GROUND_BATCH_MAX_KEYS) return WM_ERR_ARG;
    for (unsigned k = 0; k <= S; ++k) offsets_out[k] = 0;
    if (stats)
        for (unsigned k = 0; k < S; ++k) stats[k] = wm_ground_stats{};
    if (kernel_ms) *kernel_ms = 0.f;
    if (S == 0) return WM_OK;
    if (S == 1) {  // a batch of one is the single call: nothing to stage, nothing to amortise
        size_t kept = 0;
        const int rc = gs_one(ctx, scans[0].pts, scans[0].n, stride, mem, params, keep_mask, indices_out, cap, points_out,
                              out_stride, out_mem, &kept, labels_out, stats, kernel_ms);
        offsets_out[1] = kept;
        return rc;
    }
    if (C64 > (1ull << 24)) return WM_ERR_NOMEM;  // (as wm_ground_segment)
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->ground) ctx->ground = new GroundWs();
    GroundWs &g = *static_cast<GroundWs *>(ctx->ground);
    PairStage &stg = g.stage;

    GsCall c;
    gs_fill_params(params, (unsigned) C64, c.p);
    c.stride = stride;
    c.total = total;
    c.bin_blocks = (unsigned) blocks;
    c.keep = keep_mask;
    c.sc.S = S;
    c.sc.one = GsScan{nullptr, 0u, 0u, 0u, 0u};
    WM_TRY(gs_reserve(ctx, g, c, "wm_ground_segment_batch"));
    const size_t out_bytes = c.stats_len() * sizeof(unsigned long long);
    WM_TRY(stg.begin(ctx, align_up256((size_t) S * sizeof(GsScan)), cloud_bytes, 0, out_bytes, mem));
    unsigned off = 0, blk = 0;
    for (unsigned k = 0; k < S; ++k) {
        GsScan &t = stg.table<GsScan>()[k];
        t.n = (unsigned) scans[k].n;
        t.off = off;
        t.blk0 = blk;
        t.pad = 0u;
        WM_TRY(stg.up.add(ctx, scans[k].pts, scans[k].n * stride, &t.raw));
        off += t.n;
        blk += (t.n + kBlock - 1) / kBlock;
    }
    c.sc.tab = stg.d_table<GsScan>();
    c.dstats = stg.d_out.as<unsigned long long>();
    const bool host_out = out_mem == WM_MEM_HOST;
    if (labels_out && total) {
        if (host_out) {
            WM_HIP(ctx, g.labels.reserve(total));
            c.labels = g.labels.as<unsigned char>();
        } else {
            c.labels = labels_out;
        }
    }
    c.out = reinterpret_cast<int *>(indices_out);
    c.out_cap = cap;
    c.pout = static_cast<unsigned char *>(points_out);
    c.out_stride = points_out ? out_stride : 0;
    if (host_out) {  // (no more than `total` points can be kept)
        c.out_cap = std::min(cap, total);
        WM_HIP(ctx, g.out.reserve((c.out_cap ? c.out_cap : 1) * 4));
        c.out = g.out.as<int>();
        if (points_out) {
            WM_HIP(ctx, g.pts.reserve((c.out_cap ? c.out_cap : 1) * out_stride));
            c.pout = g.pts.as<unsigned char>();
        }
    }
    WM_TRY(stg.submit(ctx));
    WM_TRY(gs_front(ctx, g, c));
    const unsigned long long *hs = stg.h_out.as<unsigned long long>();
    const unsigned long long *tail = hs + (size_t) S * kGsStatsLen;
    for (int attempt = 0;; ++attempt) {
        WM_TRY(gs_back(ctx, g, c, attempt));
        WM_TRY(stg.collect(ctx, out_bytes, kernel_ms));  // the one wait (two when `mat` had to grow)
        g.mat_need = (size_t) tail[1];
        if (!tail[0]) break;
        if (attempt || g.mat.reserve(g.mat_need * sizeof(double)) != hipSuccess) {
            (void) hipGetLastError();
            ctx->last_error = "wm_ground_segment_batch: factor workspace";
            return WM_ERR_NOMEM;
        }
    }
    size_t kept = 0;
    for (unsigned k = 0; k < S; ++k) {
        kept += (size_t) hs[(size_t) k * kGsStatsLen + 9];
        offsets_out[k + 1] = kept;
        if (stats) gs_stats_out(hs + (size_t) k * kGsStatsLen, &stats[k]);
    }
    if (host_out) {
        const size_t m = std::min(kept, cap);
        if (labels_out && total) WM_HIP(ctx, hipMemcpy(labels_out, c.labels, total, hipMemcpyDeviceToHost));
        if (m) WM_HIP(ctx, hipMemcpy(indices_out, c.out, m * 4, hipMemcpyDeviceToHost));
        if (m && points_out) WM_HIP(ctx, hipMemcpy(points_out, c.pout, m * out_stride, hipMemcpyDeviceToHost));
    }
    return kept > cap ? WM_ERR_ARG : WM_OK;
}

}  // extern "C"
