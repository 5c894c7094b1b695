// wm_ground.hip -- wave::GroundSegmentation<PointT>::applyFilter on device: libwave's Gaussian-process ground filter
// (Chen et al. 2014), wave_matching/include/wave/matching/impl/ground_segmentation.hpp:10-381.
//
// One call = a few launches on the context's stream and one host wait, for the counts (a second one only when the
// factors' block has to grow, see k_gs_sector):
//   k_gs_bin       one thread per point: in range, sector, linear bin (impl :36-84); per-cell point count and the
//                  prototype (lowest z, first index) by one 64-bit atomicMin on (orderable z << 32 | index)
//   sort           (cell, index) pairs, stable (wm_sort.hpp's rs_sort_pairs): every cell's points in ascending index
//   scan           cell counts -> each cell's first place in the sorted pairs
//   k_gs_sector    one workgroup per sector (impl :108-355): signal cells (> 5 points), sorted by (height, bin),
//                  seeds, INSAC passes on a Cholesky factor of C_XX + p_sn I that grows by appended rows; per cell
//                  its kind (model / remaining / none), its rank within the sector and its reference height
//   k_gs_cells<1>  one wave per cell: labels, and per (list, sector, rank) the number of points of each list
//   scan           those counts (lists not kept count zero) -> every cell's first place in the output
//   k_gs_cells<0>  one wave per cell: the indices to their places (within a cell in input index order)
//   k_gs_finish    the counts -> the stats block the host fetches
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

#include "wm_internal.hpp"
#include "wm_sort.hpp"

namespace wm {

namespace {

constexpr int kGsThreads = 256;
constexpr int kGsStatsLen = 16;  // u64: [0..2] list sizes, [3] in range, [4] signal cells, [5] model cells,
                                 // [6] sufficient sectors, [7] passes, [8] max passes, [9] output size, [10] overflow
enum { kKindNone = 0, kKindModel = 1, kKindRest = 2 };

struct GsParams {
    double rmax, bsize_rad, bsize_lin, robot_height, max_seed_range, max_seed_height;
    double p_sf, p_sn, p_tmodel, p_tdata, coeff;  // the float parameters' values, in double
    float p_tg;
    int num_seed_points, A, L;
    unsigned C;  // A * L
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

// (sqrtf: correctly rounded, as std::sqrt(float) is on the host; HIP's __fsqrt_rn is the native approximation)
__device__ __forceinline__ float gs_xy(float x, float y) {
    return sqrtf(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
}

// impl :48-80
__global__ void __launch_bounds__(kBlock)
    k_gs_bin(const unsigned char *__restrict__ raw, size_t stride, unsigned n, GsParams p, unsigned *__restrict__ keys,
             unsigned *__restrict__ vals, unsigned *__restrict__ counts, unsigned long long *__restrict__ proto) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *q = gs_point(raw, stride, i);
    const float x = q[0], y = q[1], z = q[2];
    const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
    unsigned key = p.C;  // out of range (NaN / inf included): sorts behind every cell
    if (sqrt((double) r2) < p.rmax) {
        double ph = atan2((double) y, (double) x) * (180.0 / M_PI);
        ph = ph > 0 ? fmod(ph, 360.0) : fmod(ph + 360.0, 360.0);  // wrapTo360, wave_utils/src/math.cpp:80-87
        unsigned br = (unsigned) (ph / p.bsize_rad);
        unsigned bl = (unsigned) ((double) gs_xy(x, y) / p.bsize_lin);
        if (br >= (unsigned) p.A) br = (unsigned) p.A - 1u;  // (b)
        if (bl >= (unsigned) p.L) bl = (unsigned) p.L - 1u;
        key = br * (unsigned) p.L + bl;
        atomicAdd(&counts[key], 1u);
        atomicMin(&proto[key], ((unsigned long long) gs_orderable(z) << 32) | i);
    }
    keys[i] = key;
    vals[i] = i;
}

__device__ __forceinline__ double gs_cov(const GsParams &p, double a, double b) {  // impl :96-101
    const double d = a - b;
    return p.p_sf * exp(p.coeff * (d * d));
}

__device__ __forceinline__ bool gs_before(double ha, int ba, double hb, int bb) {  // sort by height, then bin (a)
    return ha < hb || (ha == hb && ba < bb);
}

// One workgroup per sector: impl :108-355.  The sector's slices live in HBM (num_bins_l is a user parameter);
// the factor and the per-point solves in `mat`, a block of m * m + m (m + 1) / 2 doubles taken from the bump
// counter (m = the sector's signal cells).  A sector whose block does not fit flags it (stats[10]) and skips its
// passes; the host then grows `mat` to the bump counter's total and runs the sector kernel again.
__global__ void __launch_bounds__(kGsThreads)
    k_gs_sector(const unsigned char *__restrict__ raw, size_t stride, GsParams p, const unsigned *__restrict__ counts,
                const unsigned long long *__restrict__ proto, GsSector ws, double *__restrict__ mat, size_t mat_cap,
                unsigned long long *__restrict__ bump, GsCell *__restrict__ cells, unsigned long long *__restrict__ stats) {
    __shared__ unsigned s_wave[kGsThreads / 64];
    __shared__ int s_q, s_r, s_go, s_base;
    __shared__ size_t s_off;
    const int tid = threadIdx.x, s = blockIdx.x, L = p.L;
    const size_t sl = (size_t) s * L;
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
            const size_t off = (size_t) atomicAdd(bump, (unsigned long long) need);
            if (off + need <= mat_cap) {
                s_off = off;
            } else {  // (`mat` too small: flagged, nothing written; the host grows it and runs this kernel again)
                s_go = 0;
                atomicAdd(&stats[10], 1ull);
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

// One wave per cell: its points (ascending index) are labelled 64 at a time.  COUNT: the per-(list, sector, rank)
// counts (a list that is not kept counts zero) and the lists' sizes; else the indices go to their places.
template <bool COUNT>
__global__ void __launch_bounds__(kBlock)
    k_gs_cells(const unsigned char *__restrict__ raw, size_t stride, GsParams p, const GsCell *__restrict__ cells,
               const unsigned *__restrict__ cell_start, const unsigned *__restrict__ sorted_idx, int keep,
               unsigned *__restrict__ slot, unsigned long long *__restrict__ stats, unsigned char *__restrict__ labels,
               int *__restrict__ out, size_t cap) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (c >= p.C) return;
    const GsCell ci = cells[c];
    if (ci.rank < 0) return;
    const unsigned sec = c / (unsigned) p.L;
    const size_t sidx = (size_t) sec * p.L + (size_t) ci.rank;
    const unsigned beg = cell_start[c], end = cell_start[c + 1];
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
            if (COUNT && labels) labels[pi] = (unsigned char) lab;
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const unsigned long long mk = __ballot(live && lab == l + 1);
            if (!COUNT && live && lab == l + 1 && (keep >> l) & 1) {
                const size_t o = (size_t) run[l] + (size_t) __popcll(mk & lt);
                if (o < cap) out[o] = (int) pi;
            }
            run[l] += (unsigned) __popcll(mk);
        }
    }
    if (COUNT && lane == 0) {
        for (int l = 0; l < 3; ++l) {
            slot[(size_t) l * p.C + sidx] = ((keep >> l) & 1) ? run[l] : 0u;
            if (run[l]) atomicAdd(&stats[l], (unsigned long long) run[l]);
        }
    }
}

__global__ void k_gs_finish(const unsigned *__restrict__ cell_start, const unsigned *__restrict__ slot_base, unsigned C,
                            unsigned long long *__restrict__ stats) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        stats[3] = cell_start[C];
        stats[9] = slot_base[3ull * C];
    }
}

}  // namespace

// The context's workspace of this filter: its own buffers, shared with nothing else on the context.
struct GroundWs {
    DevBuf raw, keys, vals, keys2, vals2, sort_tmp, counts, proto, cell_start, cells, slot, slot_base, sector, mat,
        stats, labels, out;
    unsigned long long *h_stats = nullptr;  // pinned
    size_t mat_need = 0;                    // doubles the sectors' factor blocks took in the last call
};

void ground_release(wm_ctx *ctx) {
    GroundWs *g = static_cast<GroundWs *>(ctx->ground);
    if (!g) return;
    DevBuf *bufs[] = {&g->raw, &g->keys, &g->vals, &g->keys2, &g->vals2, &g->sort_tmp, &g->counts, &g->proto,
                      &g->cell_start, &g->cells, &g->slot, &g->slot_base, &g->sector, &g->mat, &g->stats,
                      &g->labels, &g->out};
    for (DevBuf *b : bufs) b->release();
    if (g->h_stats) (void) hipHostFree(g->h_stats);
    delete g;
    ctx->ground = nullptr;
}

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

extern "C" {

void wm_ground_default_params(wm_ground_params *p) {
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
    const uint64_t C64 = (uint64_t) params->num_bins_a * (uint64_t) params->num_bins_l;
    if (C64 > (1ull << 24)) return WM_ERR_NOMEM;  // (a cell costs ~120 bytes of workspace)
    const unsigned C = (unsigned) C64;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->ground) ctx->ground = new GroundWs();
    GroundWs &g = *static_cast<GroundWs *>(ctx->ground);
    if (!g.h_stats) WM_HIP(ctx, hipHostMalloc((void **) &g.h_stats, kGsStatsLen * sizeof(unsigned long long), hipHostMallocDefault));
    hipStream_t st = ctx->stream;

    GsParams p;
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

    const unsigned char *raw = static_cast<const unsigned char *>(pts);
    const size_t nb = n ? n : 1;
    WM_HIP(ctx, g.keys.reserve(nb * 4));
    WM_HIP(ctx, g.vals.reserve(nb * 4));
    WM_HIP(ctx, g.keys2.reserve(nb * 4));
    WM_HIP(ctx, g.vals2.reserve(nb * 4));
    WM_HIP(ctx, g.counts.reserve((size_t) C * 4));
    WM_HIP(ctx, g.proto.reserve((size_t) C * 8));
    WM_HIP(ctx, g.cell_start.reserve(((size_t) C + 1) * 4));
    WM_HIP(ctx, g.cells.reserve((size_t) C * sizeof(GsCell)));
    WM_HIP(ctx, g.slot.reserve((size_t) 3 * C * 4));
    WM_HIP(ctx, g.slot_base.reserve(((size_t) 3 * C + 1) * 4));
    WM_HIP(ctx, g.sector.reserve((size_t) C * (6 * sizeof(double) + 5 * sizeof(int))));
    // the sectors' factor blocks (m * m + m (m + 1) / 2 doubles for m signal cells) are taken from `mat` on the device;
    // it starts at the last call's need (8 MiB at least: the fixture takes 0.5, a 1M-point ring scan 5.2) and, when a
    // sector finds it too small, grows to what the sectors asked for in all, and the sector kernel and what follows it
    // run again
    if (g.mat.reserve(std::max<size_t>(g.mat_need, (size_t) 1 << 20) * sizeof(double)) != hipSuccess) {
        (void) hipGetLastError();
        ctx->last_error = "wm_ground_segment: factor workspace";
        return WM_ERR_NOMEM;
    }
    WM_HIP(ctx, g.stats.reserve(kGsStatsLen * sizeof(unsigned long long)));
    if (mem == WM_MEM_HOST && n) {
        WM_HIP(ctx, g.raw.reserve(n * stride));
        WM_HIP(ctx, hipMemcpyAsync(g.raw.p, pts, n * stride, hipMemcpyHostToDevice, st));
        raw = g.raw.as<unsigned char>();
    }
    unsigned char *labels = nullptr;
    if (labels_out && n) {
        if (out_mem == WM_MEM_DEVICE) {
            labels = labels_out;
        } else {
            WM_HIP(ctx, g.labels.reserve(n));
            labels = g.labels.as<unsigned char>();
        }
        WM_HIP(ctx, hipMemsetAsync(labels, 0, n, st));  // WM_GROUND_NONE
    }
    int *out = reinterpret_cast<int *>(indices_out);
    size_t out_cap = cap;
    if (out_mem == WM_MEM_HOST) {
        WM_HIP(ctx, g.out.reserve(nb * 4));
        out = g.out.as<int>();
        out_cap = n;
    }
    unsigned long long *dstats = g.stats.as<unsigned long long>();
    WM_HIP(ctx, hipMemsetAsync(g.counts.p, 0, (size_t) C * 4, st));
    WM_HIP(ctx, hipMemsetAsync(g.proto.p, 0xFF, (size_t) C * 8, st));

    unsigned *keys = g.keys.as<unsigned>(), *vals = g.vals.as<unsigned>();
    unsigned *keys2 = g.keys2.as<unsigned>(), *vals2 = g.vals2.as<unsigned>();
    if (n) {
        hipLaunchKernelGGL(k_gs_bin, dim3((unsigned) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, raw, stride,
                           (unsigned) n, p, keys, vals, g.counts.as<unsigned>(), g.proto.as<unsigned long long>());
        WM_HIP(ctx, hipGetLastError());
        unsigned bits = 1;
        while (bits < 32 && (C >> bits) != 0u) ++bits;  // keys 0 .. C (C: out of range)
        WM_HIP(ctx, g.sort_tmp.reserve(rs_temp_bytes(n)));
        WM_HIP(ctx, rs_sort_pairs(g.sort_tmp.p, keys, keys2, vals, vals2, n, bits, st));
    }
    WM_TRY(exclusive_scan(ctx, g.counts.as<unsigned>(), C, g.cell_start.as<unsigned>()));

    GsSector ws;
    {
        unsigned char *b = g.sector.as<unsigned char>();
        double **d[] = {&ws.sig_r, &ws.sig_h, &ws.srt_r, &ws.srt_h, &ws.fpred, &ws.su};
        for (double **x : d) {
            *x = reinterpret_cast<double *>(b);
            b += (size_t) C * sizeof(double);
        }
        int **iv[] = {&ws.sig_b, &ws.srt_b, &ws.model, &ws.rest, &ws.inl};
        for (int **x : iv) {
            *x = reinterpret_cast<int *>(b);
            b += (size_t) C * sizeof(int);
        }
    }
    GsCell *cells = g.cells.as<GsCell>();
    const unsigned cell_blocks = (unsigned) (((size_t) C + kBlock / 64 - 1) / (kBlock / 64));
    const unsigned long long *hs = g.h_stats;
    for (int attempt = 0;; ++attempt) {
        const size_t mat_cap = g.mat.cap / sizeof(double);
        WM_HIP(ctx, hipMemsetAsync(dstats, 0, kGsStatsLen * sizeof(unsigned long long), st));
        WM_HIP(ctx, hipMemsetAsync(g.slot.p, 0, (size_t) 3 * C * 4, st));
        if (labels && attempt) WM_HIP(ctx, hipMemsetAsync(labels, 0, n, st));
        hipLaunchKernelGGL(k_gs_sector, dim3((unsigned) p.A), dim3(kGsThreads), 0, st, raw, stride, p,
                           (const unsigned *) g.counts.p, (const unsigned long long *) g.proto.p, ws, g.mat.as<double>(),
                           mat_cap, dstats + 11, cells, dstats);
        WM_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gs_cells<true>), dim3(cell_blocks), dim3(kBlock), 0, st, raw, stride, p,
                           (const GsCell *) cells, (const unsigned *) g.cell_start.p, (const unsigned *) vals2,
                           keep_mask, g.slot.as<unsigned>(), dstats, labels, (int *) nullptr, (size_t) 0);
        WM_HIP(ctx, hipGetLastError());
        WM_TRY(exclusive_scan(ctx, g.slot.as<unsigned>(), (size_t) 3 * C, g.slot_base.as<unsigned>()));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gs_cells<false>), dim3(cell_blocks), dim3(kBlock), 0, st, raw, stride, p,
                           (const GsCell *) cells, (const unsigned *) g.cell_start.p, (const unsigned *) vals2,
                           keep_mask, g.slot_base.as<unsigned>(), dstats, (unsigned char *) nullptr, out, out_cap);
        hipLaunchKernelGGL(k_gs_finish, dim3(1), dim3(64), 0, st, (const unsigned *) g.cell_start.p,
                           (const unsigned *) g.slot_base.p, C, dstats);
        WM_HIP(ctx, hipGetLastError());
        WM_HIP(ctx, hipMemcpyAsync(g.h_stats, dstats, kGsStatsLen * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   st));
        WM_HIP(ctx, hipStreamSynchronize(st));  // the one wait (two when `mat` had to grow)
        g.mat_need = (size_t) hs[11];            // (the bump counter: every sector's request, granted or not)
        if (!hs[10]) break;
        if (attempt || g.mat.reserve(g.mat_need * sizeof(double)) != hipSuccess) {
            (void) hipGetLastError();
            ctx->last_error = "wm_ground_segment: factor workspace";
            return WM_ERR_NOMEM;
        }
    }
    const size_t total = (size_t) hs[9];
    *n_out = total;
    if (stats) {
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
    if (out_mem == WM_MEM_HOST) {
        if (labels_out && n) WM_HIP(ctx, hipMemcpy(labels_out, labels, n, hipMemcpyDeviceToHost));
        if (total && cap) WM_HIP(ctx, hipMemcpy(indices_out, out, std::min(total, cap) * 4, hipMemcpyDeviceToHost));
    }
    return total > cap ? WM_ERR_ARG : WM_OK;
}

}  // extern "C"
