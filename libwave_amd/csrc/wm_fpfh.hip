// wm_fpfh.hip -- pcl::FPFHEstimation with a k-neighbourhood on the device (wm_fpfh_estimate; include/wavematch.h,
// "feature descriptors", states the rule; tests/fpfh_reference.py restates it in numpy).
//   k_fpfh_pos      where every input point stands in the query order (a list entry addresses a query, not a caller slot)
//   k_spfh<K>       one point per lane, shaped like k_normals<K>: knn_search<K>, then the pair features of the point with
//                   each neighbour; a count is at most k - 1 <= 31, so a feature's eleven bins are eleven 5-bit fields of
//                   ONE 64-bit word and a pair's increment is a shift by 5 * bin -- no register array is indexed
//                   dynamically, nothing goes to LDS or scratch.  Stores the three words in QUERY order (the grid's, or
//                   the source's Morton order: neighbours in space are neighbours in memory) and the list (position, d2).
//   k_fpfh_weight   one point per lane: its list, the neighbours' three words, 33 accumulators unpacked with constant
//                   shifts, the three sums and scales, 33 floats to the caller's slot.  It does not search.
//   k_spfh_unpack   the counts as bytes in the caller's order, only when asked for
#include "wm_fpfh_pair.hpp"
#include "wm_fpfh_ws.hpp"
#include "wm_gicp_dev.hpp"

namespace wm {

constexpr int kFpfhDefaultK = 10;
static_assert(kFpfhDim == WM_FEATURE_DIM, "the descriptor's length in the header");
constexpr int kFpfhBlock = 64;   // k_spfh: one wave per workgroup, as k_normals
constexpr int kFpfhWBlock = 256;

struct SpfhWords {
    unsigned long long f[3];
};

__global__ void __launch_bounds__(256) k_fpfh_pos(const float4 *__restrict__ qpts, unsigned nq, unsigned n_orig,
                                                  unsigned *__restrict__ pos_of) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nq) return;
    const unsigned slot = __float_as_uint(qpts[i].w);
    if (slot < n_orig) pos_of[slot] = i;
}

// (five waves per SIMD up to K = 12, where k_normals asks for six up to K = 10: under six waves' 80 registers the pair
// features on top of the search spill a few registers to scratch; under five waves' 96 nothing does)
template <int K>
__global__ void __launch_bounds__(kFpfhBlock) __attribute__((amdgpu_waves_per_eu(K <= 12 ? 5 : 1)))
    k_spfh(GridDev g, const float4 *__restrict__ qpts, unsigned nq, const float4 *__restrict__ orig, unsigned n_orig,
           const float4 *__restrict__ nrm, const unsigned *__restrict__ pos_of, int k, SpfhWords *__restrict__ words,
           uint2 *__restrict__ lists, float r0_cells) {
    __shared__ uint2 s_runs[kKnnRows * kFpfhBlock];  // per-lane run lists of knn_search (lane-private)
    const unsigned i = blockIdx.x * kFpfhBlock + threadIdx.x;
    if (i >= nq) return;
    const float4 q = qpts[i];
    const unsigned slot = __float_as_uint(q.w);
    SpfhWords w = {{0ull, 0ull, 0ull}};
    if (slot >= n_orig || !(q.x == q.x)) {  // (a non-finite point of a cloud queried in the caller's order)
        words[i] = w;
        for (int j = 0; j < k; ++j) lists[(size_t) j * nq + i] = make_uint2(i, 0u);
        return;
    }
    unsigned long long best[K];
    knn_search<K>(g, q.x, q.y, q.z, k, r0_cells, best, s_runs, threadIdx.x, kFpfhBlock);
    const float4 np = nrm[slot];
    const bool own = !(np.x == 0.f && np.y == 0.f && np.z == 0.f);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) {
            uint2 entry = make_uint2(i, 0u);  // (a short list's entry: d2 == 0 is skipped by the second pass)
            if (best[j] != ~0ull) {
                const unsigned idx = (unsigned) best[j];
                const unsigned at = idx < n_orig ? idx : slot;
                const float d2 = __uint_as_float((unsigned) (best[j] >> 32));
                entry = make_uint2(pos_of[at], __float_as_uint(d2));
                if (own && d2 != 0.f) {
                    int bin[3];
                    if (fpfh_pair(q.x, q.y, q.z, np, orig[at], nrm[at], d2, bin)) {
#pragma unroll
                        for (int f = 0; f < 3; ++f) w.f[f] += 1ull << (5 * bin[f]);
                    }
                }
            }
            lists[(size_t) j * nq + i] = entry;
        }
    }
    words[i] = w;
}

__global__ void __launch_bounds__(kFpfhWBlock)
    k_fpfh_weight(const float4 *__restrict__ qpts, unsigned nq, unsigned n_orig, const float4 *__restrict__ nrm, int k,
                  const SpfhWords *__restrict__ words, const uint2 *__restrict__ lists, float *__restrict__ out,
                  unsigned long long *__restrict__ n_valid) {
    const unsigned i = blockIdx.x * kFpfhWBlock + threadIdx.x;
    unsigned slot = ~0u;
    bool valid = false;
    if (i < nq) {
        const float4 q = qpts[i];
        slot = __float_as_uint(q.w);
        if (slot < n_orig && q.x == q.x) {
            const float4 np = nrm[slot];
            valid = !(np.x == 0.f && np.y == 0.f && np.z == 0.f);
        }
    }
    const unsigned long long vote = __ballot(valid);
    if ((threadIdx.x & 63u) == 0u && vote != 0ull) atomicAdd(n_valid, (unsigned long long) __popcll(vote));
    if (slot >= n_orig) return;
    float acc[kFpfhDim];
#pragma unroll
    for (int b = 0; b < kFpfhDim; ++b) acc[b] = 0.f;
    if (valid) {
        for (int j = 0; j < k; ++j) {
            const uint2 e = lists[(size_t) j * nq + i];
            const float d2 = __uint_as_float(e.y);
            if (d2 == 0.f) continue;
            const float wgt = __fdiv_rn(1.0f, d2);
            const SpfhWords w = words[e.x];
#pragma unroll
            for (int f = 0; f < 3; ++f)
#pragma unroll
                for (int b = 0; b < kFpfhBins; ++b)
                    acc[f * kFpfhBins + b] =
                        __fadd_rn(acc[f * kFpfhBins + b], __fmul_rn((float) (unsigned) ((w.f[f] >> (5 * b)) & 31ull), wgt));
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            float s = acc[f * kFpfhBins];
#pragma unroll
            for (int b = 1; b < kFpfhBins; ++b) s = __fadd_rn(s, acc[f * kFpfhBins + b]);
            const float scale = s != 0.f ? __fdiv_rn(100.0f, s) : 0.f;
#pragma unroll
            for (int b = 0; b < kFpfhBins; ++b) acc[f * kFpfhBins + b] = __fmul_rn(acc[f * kFpfhBins + b], scale);
        }
    }
    float *o = out + (size_t) slot * kFpfhDim;
#pragma unroll
    for (int b = 0; b < kFpfhDim; ++b) o[b] = acc[b];
}

__global__ void __launch_bounds__(256) k_spfh_unpack(const float4 *__restrict__ qpts, unsigned nq, unsigned n_orig,
                                                     const SpfhWords *__restrict__ words, unsigned char *__restrict__ counts) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nq) return;
    const unsigned slot = __float_as_uint(qpts[i].w);
    if (slot >= n_orig) return;
    const SpfhWords w = words[i];
    unsigned char *o = counts + (size_t) slot * kFpfhDim;
#pragma unroll
    for (int f = 0; f < 3; ++f)
#pragma unroll
        for (int b = 0; b < kFpfhBins; ++b) o[f * kFpfhBins + b] = (unsigned char) ((w.f[f] >> (5 * b)) & 31ull);
}

template <int K>
static int launch_spfh(wm_ctx *ctx, const GridDev &g, const float4 *q, size_t nq, const float4 *orig, size_t n_orig,
                       const float4 *nrm, const unsigned *pos_of, int k, SpfhWords *words, uint2 *lists) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_spfh<K>), dim3((unsigned) ((nq + kFpfhBlock - 1) / kFpfhBlock)), dim3(kFpfhBlock), 0,
                       ctx->stream, g, q, (unsigned) nq, orig, (unsigned) n_orig, nrm, pos_of, k, words, lists,
                       ctx->tune_knn_r0 > 0 ? ctx->tune_knn_r0 : (k <= 12 ? 1.0f : 1.5f));  // (the first radius of k_normals)
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

void fpfh_release(wm_ctx *ctx) {
    FpfhWs *w = static_cast<FpfhWs *>(ctx->fpfh);
    if (!w) return;
    DevBuf *bufs[] = {&w->pos_of, &w->words,  &w->lists,  &w->nrm_in,  &w->out,     &w->counts, &w->n_valid, &w->a,
                      &w->b,      &w->keys_a, &w->keys_b, &w->flags_a, &w->flags_b, &w->idx,    &w->d2,      &w->n_matched};
    for (DevBuf *b : bufs) b->release();
    w->h.release();
    for (hipEvent_t e : w->ev)
        if (e) (void) hipEventDestroy(e);
    delete w;
    ctx->fpfh = nullptr;
}

}  // namespace wm

using namespace wm;

extern "C" {

void wm_fpfh_default_params(wm_fpfh_params *p) {
    if (!p) return;
    p->normal_k = kFpfhDefaultK;
    p->feature_k = kFpfhDefaultK;
}

int wm_fpfh_estimate(wm_ctx *ctx, int which, const wm_fpfh_params *params, const void *normals_in, float *fpfh_out,
                     uint8_t *spfh_out, int out_mem, wm_fpfh_stats *stats) {
    if (!ctx || (which != 0 && which != 1) || !fpfh_out || (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE)) return WM_ERR_ARG;
    int normal_k = params ? params->normal_k : 0, feature_k = params ? params->feature_k : 0;
    if (normal_k == 0) normal_k = kFpfhDefaultK;
    if (feature_k == 0) feature_k = kFpfhDefaultK;
    if (normal_k < 3 || normal_k > 32 || feature_k < 3 || feature_k > 32) return WM_ERR_ARG;
    if (stats) *stats = wm_fpfh_stats{};
    if (ctx->n_src_input == 0 || ctx->n_tgt_input == 0) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(finalize_clouds(ctx));
    const size_t n_fin = which == 1 ? ctx->n_tgt : ctx->n_src, n_in = which == 1 ? ctx->n_tgt_input : ctx->n_src_input;
    if ((size_t) feature_k > n_fin || (!normals_in && (size_t) normal_k > n_fin)) return WM_NOT_CONVERGED;
    if (n_in > 0x7FFFFFF0u / kFpfhDim) return WM_ERR_ARG;
    FpfhWs *wp = fpfh_ws(ctx);
    if (!wp) return WM_ERR_HIP;
    FpfhWs &w = *wp;
    hipStream_t st = ctx->stream;

    // ---- the normals (caller order) and the grid the search scans
    // (the grid first, outside the timed stages: normals_ms is then k_normals' time, the yardstick of spfh_ms)
    const float4 *nrm = nullptr;
    if (which == 1) {
        if (!ctx->levels[0].built) WM_TRY(ensure_levels(ctx, -1.0));
    } else {
        WM_TRY(source_grid(ctx));
    }
    WM_HIP(ctx, hipEventRecord(w.ev[0], st));
    if (!normals_in) {
        if (which == 1) {
            WM_TRY(plane_target_normals(ctx, normal_k));
            nrm = ctx->plane_nrm.as<float4>();
        } else {
            WM_TRY(plane_source_normals(ctx, normal_k, true));
            nrm = ctx->plane_nrm_src.as<float4>();
        }
    } else {
        if (out_mem == WM_MEM_HOST) {
            WM_HIP(ctx, w.nrm_in.reserve(n_in * sizeof(float4)));
            WM_HIP(ctx, hipMemcpyAsync(w.nrm_in.p, normals_in, n_in * sizeof(float4), hipMemcpyHostToDevice, st));
            nrm = w.nrm_in.as<float4>();
        } else {
            nrm = static_cast<const float4 *>(normals_in);
        }
    }
    WM_HIP(ctx, hipEventRecord(w.ev[1], st));
    // the queries: the grid's own order (the target), the Morton order (the source); a target with non-finite points
    // in the caller's order, as its normals and covariances
    const GridDev &g = which == 1 ? ctx->levels[0].d : ctx->src_grid.d;
    const float4 *orig = which == 1 ? ctx->tgt_orig.as<float4>() : ctx->src_orig.as<float4>();
    const float4 *q = which == 1 ? (n_fin == n_in ? g.pts : orig) : ctx->src_sorted.as<float4>();
    const size_t nq = which == 1 && n_fin != n_in ? n_in : n_fin;

    WM_HIP(ctx, w.pos_of.reserve(n_in * sizeof(unsigned)));
    WM_HIP(ctx, w.words.reserve(nq * sizeof(SpfhWords)));
    WM_HIP(ctx, w.lists.reserve(nq * (size_t) feature_k * sizeof(uint2)));
    WM_HIP(ctx, w.n_valid.reserve(8));
    WM_HIP(ctx, w.h.reserve(8));
    float *d_out = fpfh_out;
    unsigned char *d_counts = spfh_out;
    if (out_mem == WM_MEM_HOST) {
        WM_HIP(ctx, w.out.reserve(n_in * kFpfhDim * sizeof(float)));
        d_out = w.out.as<float>();
        if (spfh_out) {
            WM_HIP(ctx, w.counts.reserve(n_in * kFpfhDim));
            d_counts = w.counts.as<unsigned char>();
        }
    }
    WM_HIP(ctx, hipMemsetAsync(w.n_valid.p, 0, 8, st));
    if (nq != n_in) {  // (points that are no query keep zeros)
        WM_HIP(ctx, hipMemsetAsync(w.pos_of.p, 0, n_in * sizeof(unsigned), st));
        WM_HIP(ctx, hipMemsetAsync(d_out, 0, n_in * kFpfhDim * sizeof(float), st));
        if (d_counts) WM_HIP(ctx, hipMemsetAsync(d_counts, 0, n_in * kFpfhDim, st));
    }
    const unsigned blocks256 = (unsigned) ((nq + 255) / 256);
    hipLaunchKernelGGL(k_fpfh_pos, dim3(blocks256), dim3(256), 0, st, q, (unsigned) nq, (unsigned) n_in, w.pos_of.as<unsigned>());
    WM_HIP(ctx, hipGetLastError());
    WM_TRY(knn_ladder(feature_k, [&](auto K) {
        return launch_spfh<decltype(K)::value>(ctx, g, q, nq, orig, n_in, nrm, w.pos_of.as<unsigned>(), feature_k,
                                               w.words.as<SpfhWords>(), w.lists.as<uint2>());
    }));
    WM_HIP(ctx, hipEventRecord(w.ev[2], st));
    hipLaunchKernelGGL(k_fpfh_weight, dim3((unsigned) ((nq + kFpfhWBlock - 1) / kFpfhWBlock)), dim3(kFpfhWBlock), 0, st, q,
                       (unsigned) nq, (unsigned) n_in, nrm, feature_k, w.words.as<SpfhWords>(), w.lists.as<uint2>(), d_out,
                       w.n_valid.as<unsigned long long>());
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipEventRecord(w.ev[3], st));
    if (d_counts) {
        hipLaunchKernelGGL(k_spfh_unpack, dim3(blocks256), dim3(256), 0, st, q, (unsigned) nq, (unsigned) n_in,
                           w.words.as<SpfhWords>(), d_counts);
        WM_HIP(ctx, hipGetLastError());
    }
    WM_HIP(ctx, hipMemcpyAsync(w.h.p, w.n_valid.p, 8, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (stats) {
        stats->n_valid = (size_t) *w.h.as<unsigned long long>();
        if (!normals_in) (void) hipEventElapsedTime(&stats->normals_ms, w.ev[0], w.ev[1]);
        (void) hipEventElapsedTime(&stats->spfh_ms, w.ev[1], w.ev[2]);
        (void) hipEventElapsedTime(&stats->weight_ms, w.ev[2], w.ev[3]);
    }
    if (out_mem == WM_MEM_HOST) {
        WM_TRY(copy_to_caller(ctx, fpfh_out, d_out, n_in * kFpfhDim * sizeof(float)));
        if (spfh_out) WM_TRY(copy_to_caller(ctx, spfh_out, d_counts, n_in * kFpfhDim));
    }
    return WM_OK;
}

}  // extern "C"
