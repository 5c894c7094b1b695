// wm_plane.hip -- the point-to-plane error metric of ICP (wm_icp_params.mode == WM_ICP_PLANE): what
// pcl::IterativeClosestPointWithNormals adds to pcl::IterativeClosestPoint (normals of the target from
// pcl::NormalEstimation, TransformationEstimationPointToPlaneLLS's residual n . (p - q)); libwave's ICPMatcher
// (wave_matching/src/icp.cpp) has no counterpart -- an opt-in of this library.
//   k_normals<K>    a normal and a curvature per point of a cloud from its k nearest neighbours in the same cloud (the
//                   neighbourhood of k_gicp_cov: knn_search<K>, same keys, same tie order)
//   k_plane_stats   one streaming pass over the queries after a search-only launch: the 29 sums of the public GN layout
//                   with the plane residual, into bins of exact integer limbs (wm_bins.hpp)
//   k_plane_solve   the bins added up, the degeneracy test, gn6_from_stats and the unchanged stopping rules
//                   (icp_apply_stats), the record for the host
// The loop that launches them is icp_run_loop's (wm_icp.hip).
#include "wm_internal.hpp"
#include "wm_icp_step.hpp"
#include "wm_bins.hpp"
#include "wm_gicp_dev.hpp"
#include "wm_normal_rule.hpp"
#include "wm_pair_terms.hpp"

#include <string.h>

namespace wm {

// ------------------------------------------------------------------ normals
// One query per lane, ONE wave per workgroup, as k_gicp_cov (whose measurements chose that shape: the search is a chain
// of dependent look-ups per wave, what counts is how many waves are resident and how soon a finished one is replaced).
// The covariance is formed in f64 from the differences to the query point (exact in f64 for float coordinates up to a
// 2^29 range ratio), then taken about their mean: the same matrix as the covariance about the neighbourhood mean, with
// no cancellation against the cloud's offset from the origin.  Its eigenvectors are the right singular vectors of the
// symmetric matrix (svd3<false>: IEEE operations only; V stays orthonormal when an eigenvalue is zero).
constexpr int kNrmBlock = 64;
template <int K>
__global__ void __launch_bounds__(kNrmBlock) __attribute__((amdgpu_waves_per_eu(K <= 10 ? 6 : (K <= 12 ? 5 : 1))))
    k_normals(GridDev g, const float4 *__restrict__ qpts, unsigned n, const float4 *__restrict__ orig, unsigned n_orig, int k,
              float4 *__restrict__ out, float r0_cells) {
    __shared__ uint2 s_runs[kKnnRows * kNrmBlock];  // per-lane run lists of knn_search (lane-private)
    const unsigned i = blockIdx.x * kNrmBlock + threadIdx.x;
    if (i >= n) return;
    const float4 q = qpts[i];
    const unsigned slot = __float_as_uint(q.w);
    if (slot >= n_orig) return;
    if (!(q.x == q.x)) {  // (no such point is in a grid or a sorted cloud; the output was zeroed)
        out[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    unsigned long long best[K];
    knn_search<K>(g, q.x, q.y, q.z, k, r0_cells, best, s_runs, threadIdx.x, kNrmBlock);
    double s[3] = {0, 0, 0}, c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int found = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k && best[j] != ~0ull) {
            const unsigned idx = (unsigned) best[j];
            const float4 p = orig[idx < n_orig ? idx : slot];
            const double dx = (double) p.x - (double) q.x, dy = (double) p.y - (double) q.y, dz = (double) p.z - (double) q.z;
            s[0] += dx;
            s[1] += dy;
            s[2] += dz;
            c[0] += dx * dx;
            c[3] += dy * dx;
            c[4] += dy * dy;
            c[6] += dz * dx;
            c[7] += dz * dy;
            c[8] += dz * dz;
            ++found;
        }
    }
    float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
    if (found == k) {  // (a cloud of fewer than k points is refused by the host)
        const double kk = (double) k;
#pragma unroll
        for (int a = 0; a < 3; ++a) s[a] /= kk;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
                if (b <= a) {
                    c[a * 3 + b] = c[a * 3 + b] / kk - s[a] * s[b];
                    c[b * 3 + a] = c[a * 3 + b];
                }
        float r[4];
        normal_finish(c, q.x, q.y, q.z, r);  // (wm_normal_rule.hpp: the finish the radius form shares)
        res = make_float4(r[0], r[1], r[2], r[3]);
    }
    out[slot] = res;
}

template <int K>
static int launch_normals(wm_ctx *ctx, const GridDev &g, const float4 *q, size_t n, const float4 *orig, size_t n_orig, int k,
                          float4 *out) {
    if (n == 0) return WM_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_normals<K>), dim3((unsigned) ((n + kNrmBlock - 1) / kNrmBlock)), dim3(kNrmBlock), 0,
                       ctx->stream, g, q, (unsigned) n, orig, (unsigned) n_orig, k, out,
                       ctx->tune_knn_r0 > 0 ? ctx->tune_knn_r0 : (k <= 12 ? 1.0f : 1.5f));
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// (the K ladder of the covariance kernel: the smallest instantiated list that holds k)
static int launch_normals_k(wm_ctx *ctx, const GridDev &g, const float4 *q, size_t n, const float4 *orig, size_t n_orig, int k,
                            float4 *out) {
    return knn_ladder(k, [&](auto K) { return launch_normals<decltype(K)::value>(ctx, g, q, n, orig, n_orig, k, out); });
}

int plane_normal_k(int k) { return k == 0 ? kPlaneDefaultK : k; }

// the target's normals (caller order: what a key's index addresses), estimated once per target and k
int plane_target_normals(wm_ctx *ctx, int k) {
    k = plane_normal_k(k);
    if (k < 3 || k > 32) return WM_ERR_ARG;
    if (ctx->plane_nrm_valid && ctx->plane_nrm_k == k) return WM_OK;
    if ((size_t) k > ctx->n_tgt) return WM_NOT_CONVERGED;  // (as PCL's GICP with fewer points than neighbours: no alignment)
    if (!ctx->levels[0].built) WM_TRY(ensure_levels(ctx, -1.0));
    const size_t n_in = ctx->n_tgt_input;
    WM_HIP(ctx, ctx->plane_nrm.reserve((n_in + 1) * sizeof(float4)));
    // (non-finite points are in no grid: their normals stay zero)
    if (ctx->n_tgt != n_in) WM_HIP(ctx, hipMemsetAsync(ctx->plane_nrm.p, 0, n_in * sizeof(float4), ctx->stream));
    const GridDev &g = ctx->levels[0].d;
    WM_TRY(launch_normals_k(ctx, g, g.pts, ctx->n_tgt, ctx->tgt_orig.as<float4>(), n_in, k, ctx->plane_nrm.as<float4>()));
    ctx->plane_nrm_valid = true;
    ctx->plane_nrm_k = k;
    return WM_OK;
}

// the source's normals (caller order) into ctx->plane_nrm_src, over the source's own grid (left built on ctx->src_grid);
// k is already resolved (plane_normal_k or the caller's own default); grid_ready: the caller has just built that grid
int plane_source_normals(wm_ctx *ctx, int k, bool grid_ready) {
    if (k < 3 || k > 32) return WM_ERR_ARG;
    if ((size_t) k > ctx->n_src) return WM_NOT_CONVERGED;
    const size_t n_out = ctx->n_src_input;
    WM_HIP(ctx, ctx->plane_nrm_src.reserve((n_out + 1) * sizeof(float4)));
    WM_HIP(ctx, hipMemsetAsync(ctx->plane_nrm_src.p, 0, n_out * sizeof(float4), ctx->stream));
    if (!grid_ready) WM_TRY(source_grid(ctx));  // wm_gicp.hip: the grid over the source that its covariances search
    return launch_normals_k(ctx, ctx->src_grid.d, ctx->src_sorted.as<float4>(), ctx->n_src, ctx->src_orig.as<float4>(), n_out, k,
                            ctx->plane_nrm_src.as<float4>());
}

// ------------------------------------------------------------------ the plane sums
// The 29 sums in the public GN layout (kGnN, kGnSd2, kGnH, kGnG).  A streaming kernel: per query 16 B of source point,
// 8 B of key, 16 B of matched point and one 16-B gather of the match's normal out of a table the cache holds (16 MB at
// 1M points) -- 56 B, 56 MB per pass at 1M queries, ~10 us at the measured copy rate.  kPlaneUnroll queries per thread
// and trip, every load issued before the first use.  Per-wave sums by recursive halving in a fixed lane order, the four
// waves of a workgroup added in wave order, the workgroup's 29 totals into the bins as exact integer limbs: the result
// does not depend on the order the workgroups finish in.
constexpr int kPlaneComps = 29;
constexpr int kPlaneUnroll = 4;
constexpr int kPlaneMaxBlocks = 1024;
static_assert(kGnG + 6 == kPlaneComps && kPlaneComps < (int) kBinPoison, "the GN layout inside a bin's limb row");

__global__ void __launch_bounds__(kBlock)
    k_plane_stats(const float4 *__restrict__ src, unsigned n, const unsigned long long *__restrict__ keys,
                  const float4 *__restrict__ match_pt, const float4 *__restrict__ normals, unsigned n_normals,
                  const IcpDevState *__restrict__ st, long long *__restrict__ bins, const int *__restrict__ rej) {
    if (st->done) return;
    // correspondence rejection (wm_reject.hip): a matched pair counts iff its d2's bit pattern is <= the threshold's
    // (signed: "reject everything" is a negative one); no rejection: no d2 is above INT_MAX
    const int rej_thr = rej ? *rej : 0x7FFFFFFF;
    double a[kPlaneComps];
#pragma unroll
    for (int k = 0; k < kPlaneComps; ++k) a[k] = 0.0;
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = st->Tf[k];
    const unsigned stride = gridDim.x * kBlock;
    for (unsigned i0 = blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kPlaneUnroll * stride) {
        float4 pv[kPlaneUnroll], qv[kPlaneUnroll], nv[kPlaneUnroll];
        unsigned long long keyv[kPlaneUnroll];
#pragma unroll
        for (int u = 0; u < kPlaneUnroll; ++u) {
            const unsigned i = i0 + u * stride;
            const unsigned ic = i < n ? i : i0;
            pv[u] = src[ic];
            keyv[u] = keys[ic];
            qv[u] = match_pt[ic];
        }
#pragma unroll
        for (int u = 0; u < kPlaneUnroll; ++u) {
            const unsigned idx = (unsigned) keyv[u];
            nv[u] = normals[idx < n_normals ? idx : 0u];  // (unmatched: any line; not used)
        }
#pragma unroll
        for (int u = 0; u < kPlaneUnroll; ++u) {
            if (i0 + u * stride >= n) break;
            const unsigned long long key = keyv[u];
            const unsigned idx = (unsigned) key;
            if (idx >= n_normals) continue;  // kNoIdx: no match within max_corr
            if ((int) (unsigned) (key >> 32) > rej_thr) continue;  // rejected
            // the source point under the pose the search used: the search kernels' float arithmetic
            const float4 p4 = pv[u];
            float fx, fy, fz;
            xform_pcl(T, p4.x, p4.y, p4.z, fx, fy, fz);
            a[kGnN] += 1.0;
            a[kGnSd2] += (double) __uint_as_float((unsigned) (key >> 32));  // the search's own d2, as the other modes' MSE
            const float4 n4 = nv[u];
            if (n4.x == 0.f && n4.y == 0.f && n4.z == 0.f) continue;  // no normal: counts for the MSE only
            const double px = fx, py = fy, pz = fz;
            const double J[6] = {(double) n4.x, (double) n4.y, (double) n4.z,
                                 py * (double) n4.z - pz * (double) n4.y,
                                 pz * (double) n4.x - px * (double) n4.z,
                                 px * (double) n4.y - py * (double) n4.x};
            const double r = J[0] * (px - (double) qv[u].x) + J[1] * (py - (double) qv[u].y) + J[2] * (pz - (double) qv[u].z);
            int k = kGnH;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) a[k++] += J[i] * J[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) a[kGnG + i] += J[i] * r;
        }
    }
#pragma unroll
    for (int k = 0; k < kPlaneComps; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_down(a[k], off);
    __shared__ double lds[kBlock / 64][kPlaneComps];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < kPlaneComps; ++k) lds[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x < kPlaneComps) {
        double s = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += lds[w][threadIdx.x];
        bins_add(bins, blockIdx.x % (unsigned) kBinCount, threadIdx.x, s);
    }
}

int plane_bins_ready(wm_ctx *ctx) {  // the plane pass's own bins: zero before an iteration loop, kept zero by its solve
    WM_HIP(ctx, ctx->plane_bins.reserve(kBinWords * sizeof(long long)));
    WM_HIP(ctx, hipMemsetAsync(ctx->plane_bins.p, 0, kBinWords * sizeof(long long), ctx->stream));
    return WM_OK;
}

int launch_plane_stats(wm_ctx *ctx, const int *rej) {
    const unsigned n = (unsigned) ctx->n_src;
    if (n == 0) return WM_OK;
    if (!ctx->plane_bins.p || !ctx->plane_nrm_valid) return WM_ERR_STATE;
    unsigned blocks = (n + kBlock * kPlaneUnroll - 1) / (kBlock * kPlaneUnroll);
    if (blocks > (unsigned) kPlaneMaxBlocks) blocks = kPlaneMaxBlocks;
    hipLaunchKernelGGL(k_plane_stats, dim3(blocks), dim3(kBlock), 0, ctx->stream, ctx->src_sorted.as<float4>(), n,
                       ctx->keys.as<unsigned long long>(), ctx->match_pt.as<float4>(), ctx->plane_nrm.as<float4>(),
                       (unsigned) ctx->n_tgt_input, ctx->d_state.as<IcpDevState>(), ctx->plane_bins.as<long long>(), rej);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// ------------------------------------------------------------------ the solve
// J^T J is singular when the matched normals leave a motion free (one plane: three of them).  The Cholesky pivots say so:
// pivot i is what row i of J^T J still holds once the rows before it are eliminated.  A pivot that is not above
// kPlanePivotTol x the largest diagonal entry is at the rounding level of the elimination (6 x 6, f64: a few 1e-16 of the
// largest entry; the sums themselves are exact across waves) -- 1e-12 leaves four decimal digits above that and is
// eight below what any geometry that constrains the motion gives (a wall patch of 1 % of the points: 1e-4).
constexpr double kPlanePivotTol = 1e-12;
__host__ __device__ inline bool plane_degenerate(const double *st) {
    double A[36], L[36], dmax = 0.0;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            A[i * 6 + j] = A[j * 6 + i] = st[kGnH + k];
            ++k;
        }
    for (int i = 0; i < 6; ++i) dmax = fmax(dmax, A[i * 7]);
    if (!(dmax > 0.0)) return true;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[i * 6 + j];
            for (int m = 0; m < j; ++m) s -= L[i * 6 + m] * L[j * 6 + m];
            if (i == j) {
                if (!(s > kPlanePivotTol * dmax)) return true;
                L[i * 6 + i] = sqrt(s);
            } else {
                L[i * 6 + j] = s / L[j * 6 + j];
            }
        }
    return false;
}

// One workgroup, as k_bins_solve: the state and the bins in one round trip, the bins' words added and zeroed, thread 0
// solves and publishes.  solve == 0 (wm_icp_stats_for): the sums are left in st->stats, nothing else.
__global__ void __launch_bounds__(kBlock)
    k_plane_solve(long long *__restrict__ bins, IcpDevState *st, unsigned long long *pub, int pub_slots, unsigned n_src, int solve) {
    __shared__ IcpDevState s_st;
    __shared__ BinsLdsT<kPlaneComps> s_b;
    static_assert(sizeof(IcpDevState) % 4 == 0, "word-wise staging");
    constexpr unsigned kWords = sizeof(IcpDevState) / 4;
    for (unsigned w = threadIdx.x; w < kWords; w += kBlock) reinterpret_cast<unsigned *>(&s_st)[w] = reinterpret_cast<const unsigned *>(st)[w];
    bins_collect<kBlock, kPlaneComps, kPlaneComps>(bins, s_b);  // (ends with a barrier)
    if (s_st.done) return;  // (uniform; queued behind a `done`: the bins were zero and stay so)
    if (threadIdx.x == 0) {
        double ex[kStatsLen];
#pragma unroll
        for (int k = 0; k < kStatsLen; ++k) ex[k] = 0.0;
        if (!s_b.poison)  // (poisoned: a sum the limbs cannot hold -> "no correspondences", loud, not wrong)
            for (int k = 0; k < kPlaneComps; ++k) ex[k] = s_b.tot[k];
        ex[kStatsLen - 1] = (double) n_src;  // source points handled: all of them (no sharding in this mode)
        s_st.local_handled = ex[kStatsLen - 1];
        for (int k = 0; k < kStatsLen; ++k) s_st.stats[k] = ex[k];
        if (solve) {
            if (ex[kGnN] >= 3.0 && plane_degenerate(ex)) {
                // no step: the pose, and with it T_out, stay as they are
                for (int k = 0; k < 12; ++k) s_st.Tf_search[k] = s_st.Tf[k];
                s_st.n_corr = (int) ex[kGnN];
                s_st.mse = ex[kGnSd2] / ex[kGnN];
                s_st.deferred_total += s_st.queue_count[1];
                for (int l = 0; l <= kMaxLevels; ++l) s_st.queue_count[l] = 0;
                for (int k = 0; k < 64; ++k) s_st.cert_unsettled[k] = 0u;
                s_st.state = WM_CONV_DEGENERATE;
                s_st.converged = 0;
                s_st.done = 1;
            } else {
                icp_apply_stats(&s_st, ex);
            }
            publish_step(&s_st, pub, pub_slots);
        }
    }
    __syncthreads();
    for (unsigned w = threadIdx.x; w < kWords; w += kBlock) reinterpret_cast<unsigned *>(st)[w] = reinterpret_cast<const unsigned *>(&s_st)[w];
}

int launch_plane_solve(wm_ctx *ctx, unsigned long long *pub, int pub_slots, int solve) {
    hipLaunchKernelGGL(k_plane_solve, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->plane_bins.as<long long>(),
                       ctx->d_state.as<IcpDevState>(), pub, pub_slots, (unsigned) ctx->n_src, solve);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

}  // namespace wm

using namespace wm;

extern "C" int wm_estimate_normals(wm_ctx *ctx, int which, int k, void *normals_out, int out_mem) {
    if (!ctx || (which != 0 && which != 1) || !normals_out || (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE)) return WM_ERR_ARG;
    k = plane_normal_k(k);
    if (k < 3 || k > 32) return WM_ERR_ARG;
    if (ctx->n_src_input == 0 || ctx->n_tgt_input == 0) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(finalize_clouds(ctx));
    const float4 *res = nullptr;
    size_t n_out = 0;
    if (which == 1) {
        WM_TRY(plane_target_normals(ctx, k));
        res = ctx->plane_nrm.as<float4>();
        n_out = ctx->n_tgt_input;
    } else {
        WM_TRY(plane_source_normals(ctx, k));
        n_out = ctx->n_src_input;
        res = ctx->plane_nrm_src.as<float4>();
    }
    if (out_mem == WM_MEM_DEVICE) {
        WM_HIP(ctx, hipMemcpyAsync(normals_out, res, n_out * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
        WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WM_OK;
    }
    return copy_to_caller(ctx, normals_out, res, n_out * sizeof(float4));
}
