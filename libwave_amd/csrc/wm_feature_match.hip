// wm_feature_match.hip -- nearest-descriptor correspondences (wm_feature_match; include/wavematch.h, "feature
// descriptors": pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33> and its reciprocal
// variant), all pairs, exact float32 squared distances accumulated in bin order.
//   k_feat_flags    per row: is any of its 33 floats not zero (a zero row has no match and is nobody's match)
//   k_feat_match    a lane keeps kFmRows rows of A in registers; tiles of B go through LDS and are read as broadcasts,
//                   four bins per ds_read_b128 (a row is padded to 36 floats; the 34th carries the row's flag); direct
//                   differences, 99 vector operations per pair -- plain VALU work: FP32 MFMA has the vector unit's
//                   rate on this part, and |a|^2 + |b|^2 - 2 a.b cancels and would not give the rule's bits.  Per
//                   A row and LDS cycle: 9 reads of 4 cycles per 2 x 99 operations of 2 cycles, a third of the array's
//                   rate with four waves of a CU in the loop.  The best (d2 bits << 32 | j) is a 64-bit key as
//                   g_make_key's (d2 >= 0 orders as unsigned); B is split over blockIdx.y so that a small A still
//                   fills the device, and the splits' keys meet in a 64-bit atomicMin: a minimum, hence deterministic.
//   k_feat_finish   keys -> (index, d2); reciprocal: the same match kernel with the roles exchanged, compared here
#include "wm_fpfh_ws.hpp"
#include "wm_gicp_dev.hpp"

namespace wm {

constexpr int kFmDim = WM_FEATURE_DIM;
constexpr int kFmPad = 36;      // floats per row in LDS: nine float4
constexpr int kFmBlock = 256;
constexpr int kFmRows = 2;      // rows of A per lane
constexpr int kFmTile = 128;    // rows of B per tile: 18 KB of LDS
constexpr unsigned kFmTargetBlocks = 1024;  // workgroups a launch aims at: four per compute unit

__global__ void __launch_bounds__(256) k_feat_flags(const float *__restrict__ rows, unsigned n, unsigned stride_f,
                                                    unsigned char *__restrict__ flags) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *r = rows + (size_t) i * stride_f;
    bool any = false;
#pragma unroll
    for (int b = 0; b < kFmDim; ++b) any |= r[b] != 0.f;
    flags[i] = any ? 1 : 0;
}

// keys[i] = min over this workgroup's tiles of B of (d2(i, j) bits << 32 | j), j a row of B whose flag is set
__global__ void __launch_bounds__(kFmBlock)
    k_feat_match(const float *__restrict__ a, unsigned na, unsigned a_stride_f, const float *__restrict__ b, unsigned nb,
                 unsigned b_stride_f, const unsigned char *__restrict__ b_flags, unsigned tiles_per_split,
                 unsigned long long *__restrict__ keys) {
    __shared__ float4 s_tile[kFmTile * (kFmPad / 4)];
    float *s_f = reinterpret_cast<float *>(s_tile);
    const unsigned row0 = blockIdx.x * (kFmBlock * kFmRows) + threadIdx.x;
    float ar[kFmRows][kFmDim];
    unsigned long long best[kFmRows];
#pragma unroll
    for (int r = 0; r < kFmRows; ++r) {
        const unsigned row = row0 + r * kFmBlock;
        const float *src = a + (size_t) (row < na ? row : na - 1) * a_stride_f;  // (a lane past the end computes, stores nothing)
#pragma unroll
        for (int c = 0; c < kFmDim; ++c) ar[r][c] = src[c];
        best[r] = ~0ull;
    }
    const unsigned n_tiles = (nb + kFmTile - 1) / kFmTile;
    const unsigned t0 = blockIdx.y * tiles_per_split, t1 = min(t0 + tiles_per_split, n_tiles);
    for (unsigned t = t0; t < t1; ++t) {
        const unsigned j0 = t * kFmTile, cnt = min((unsigned) kFmTile, nb - j0);
        __syncthreads();  // (the previous tile has been read)
        for (unsigned e = threadIdx.x; e < cnt * kFmDim; e += kFmBlock) {
            const unsigned r = e / kFmDim, c = e - r * kFmDim;
            s_f[r * kFmPad + c] = b[(size_t) (j0 + r) * b_stride_f + c];
        }
        if (threadIdx.x < cnt) s_f[threadIdx.x * kFmPad + kFmDim] = b_flags[j0 + threadIdx.x] ? 1.f : 0.f;
        __syncthreads();
        for (unsigned r = 0; r < cnt; ++r) {
            const float4 *row = s_tile + r * (kFmPad / 4);
            float d[kFmRows];
#pragma unroll
            for (int q = 0; q < kFmRows; ++q) d[q] = 0.f;
            float4 v;
#pragma unroll
            for (int c4 = 0; c4 < kFmDim / 4; ++c4) {
                v = row[c4];
                const float tv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int q = 0; q < kFmRows; ++q) {
                        const float df = __fsub_rn(ar[q][c4 * 4 + u], tv[u]);
                        d[q] = __fadd_rn(d[q], __fmul_rn(df, df));
                    }
            }
            v = row[kFmDim / 4];  // bin 32 and the row's flag
#pragma unroll
            for (int q = 0; q < kFmRows; ++q) {
                const float df = __fsub_rn(ar[q][kFmDim - 1], v.x);
                d[q] = __fadd_rn(d[q], __fmul_rn(df, df));
                const unsigned long long key = v.y != 0.f ? g_make_key(d[q], j0 + r) : ~0ull;
                best[q] = key < best[q] ? key : best[q];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kFmRows; ++r) {
        const unsigned row = row0 + r * kFmBlock;
        if (row < na && best[r] != ~0ull) atomicMin(&keys[row], best[r]);
    }
}

__global__ void __launch_bounds__(256)
    k_feat_finish(const unsigned long long *__restrict__ keys_a, const unsigned char *__restrict__ a_flags, unsigned na,
                  const unsigned long long *__restrict__ keys_b /* reciprocal, else null */, unsigned nb, int *__restrict__ idx_out,
                  float *__restrict__ d2_out, unsigned long long *__restrict__ n_matched) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    bool matched = false;
    if (i < na) {
        const unsigned long long key = keys_a[i];
        int j = -1;
        if (a_flags[i] && key != ~0ull && (unsigned) key < nb) {
            j = (int) (unsigned) key;
            if (keys_b && (unsigned) keys_b[j] != i) j = -1;
        }
        matched = j >= 0;
        idx_out[i] = j;
        if (d2_out) d2_out[i] = matched ? __uint_as_float((unsigned) (key >> 32)) : 0.f;
    }
    const unsigned long long vote = __ballot(matched);
    if ((threadIdx.x & 63u) == 0u && vote != 0ull) atomicAdd(n_matched, (unsigned long long) __popcll(vote));
}

// keys (n_q entries, preset to all ones) of the rows `q` against the rows `t`
static int launch_match(wm_ctx *ctx, const float *q, size_t n_q, size_t q_stride_f, const float *t, size_t n_t, size_t t_stride_f,
                        const unsigned char *t_flags, unsigned long long *keys) {
    WM_HIP(ctx, hipMemsetAsync(keys, 0xFF, n_q * sizeof(unsigned long long), ctx->stream));
    if (n_q == 0 || n_t == 0) return WM_OK;
    const unsigned bx = (unsigned) ((n_q + kFmBlock * kFmRows - 1) / (kFmBlock * kFmRows));
    const unsigned n_tiles = (unsigned) ((n_t + kFmTile - 1) / kFmTile);
    unsigned splits = (kFmTargetBlocks + bx - 1) / bx;
    splits = splits < 1u ? 1u : (splits > n_tiles ? n_tiles : splits);
    const unsigned per = (n_tiles + splits - 1) / splits;
    splits = (n_tiles + per - 1) / per;
    hipLaunchKernelGGL(k_feat_match, dim3(bx, splits), dim3(kFmBlock), 0, ctx->stream, q, (unsigned) n_q, (unsigned) q_stride_f, t,
                       (unsigned) n_t, (unsigned) t_stride_f, t_flags, per, keys);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

}  // namespace wm

using namespace wm;

extern "C" int wm_feature_match(wm_ctx *ctx, const void *a, size_t na, size_t a_stride_bytes, const void *b, size_t nb,
                                size_t b_stride_bytes, int mem, int reciprocal, int32_t *idx_out, float *d2_out, int out_mem,
                                wm_feature_match_stats *stats) {
    const size_t row_bytes = kFmDim * sizeof(float);
    if (!ctx || !idx_out || (mem != WM_MEM_HOST && mem != WM_MEM_DEVICE) || (out_mem != WM_MEM_HOST && out_mem != WM_MEM_DEVICE))
        return WM_ERR_ARG;
    if (a_stride_bytes < row_bytes || a_stride_bytes % 4 != 0 || b_stride_bytes < row_bytes || b_stride_bytes % 4 != 0) return WM_ERR_ARG;
    if (a_stride_bytes > 0xFFFFFFFFu || b_stride_bytes > 0xFFFFFFFFu) return WM_ERR_ARG;
    if (na > WM_FEATURE_MAX_ROWS || nb > WM_FEATURE_MAX_ROWS || (na > 0 && !a) || (nb > 0 && !b)) return WM_ERR_ARG;
    if (stats) *stats = wm_feature_match_stats{};
    if (na == 0) return WM_OK;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    FpfhWs *wp = fpfh_ws(ctx);
    if (!wp) return WM_ERR_HIP;
    FpfhWs &w = *wp;
    hipStream_t st = ctx->stream;
    const float *d_a = static_cast<const float *>(a), *d_b = static_cast<const float *>(b);
    if (mem == WM_MEM_HOST) {
        // (the last record may end with its row: nothing behind the 33 floats is read)
        const size_t a_bytes = (na - 1) * a_stride_bytes + row_bytes, b_bytes = nb ? (nb - 1) * b_stride_bytes + row_bytes : 0;
        WM_HIP(ctx, w.a.reserve(a_bytes));
        WM_HIP(ctx, hipMemcpyAsync(w.a.p, a, a_bytes, hipMemcpyHostToDevice, st));
        d_a = w.a.as<float>();
        if (nb) {
            WM_HIP(ctx, w.b.reserve(b_bytes));
            WM_HIP(ctx, hipMemcpyAsync(w.b.p, b, b_bytes, hipMemcpyHostToDevice, st));
            d_b = w.b.as<float>();
        }
    }
    WM_HIP(ctx, w.keys_a.reserve(na * 8));
    WM_HIP(ctx, w.keys_b.reserve((nb ? nb : 1) * 8));
    WM_HIP(ctx, w.flags_a.reserve(na));
    WM_HIP(ctx, w.flags_b.reserve(nb ? nb : 1));
    WM_HIP(ctx, w.n_matched.reserve(8));
    WM_HIP(ctx, w.h.reserve(8));
    int *d_idx = idx_out;
    float *d_d2 = d2_out;
    if (out_mem == WM_MEM_HOST) {
        WM_HIP(ctx, w.idx.reserve(na * 4));
        d_idx = w.idx.as<int>();
        if (d2_out) {
            WM_HIP(ctx, w.d2.reserve(na * 4));
            d_d2 = w.d2.as<float>();
        }
    }
    const unsigned a_sf = (unsigned) (a_stride_bytes / 4), b_sf = (unsigned) (b_stride_bytes / 4);
    WM_HIP(ctx, hipEventRecord(w.ev[0], st));
    WM_HIP(ctx, hipMemsetAsync(w.n_matched.p, 0, 8, st));
    hipLaunchKernelGGL(k_feat_flags, dim3((unsigned) ((na + 255) / 256)), dim3(256), 0, st, d_a, (unsigned) na, a_sf,
                       w.flags_a.as<unsigned char>());
    WM_HIP(ctx, hipGetLastError());
    if (nb) {
        hipLaunchKernelGGL(k_feat_flags, dim3((unsigned) ((nb + 255) / 256)), dim3(256), 0, st, d_b, (unsigned) nb, b_sf,
                           w.flags_b.as<unsigned char>());
        WM_HIP(ctx, hipGetLastError());
    }
    WM_TRY(launch_match(ctx, d_a, na, a_sf, d_b, nb, b_sf, w.flags_b.as<unsigned char>(), w.keys_a.as<unsigned long long>()));
    const bool recip = reciprocal != 0 && nb > 0;
    if (recip)
        WM_TRY(launch_match(ctx, d_b, nb, b_sf, d_a, na, a_sf, w.flags_a.as<unsigned char>(), w.keys_b.as<unsigned long long>()));
    hipLaunchKernelGGL(k_feat_finish, dim3((unsigned) ((na + 255) / 256)), dim3(256), 0, st, w.keys_a.as<unsigned long long>(),
                       w.flags_a.as<unsigned char>(), (unsigned) na, recip ? w.keys_b.as<unsigned long long>() : nullptr, (unsigned) nb,
                       d_idx, d_d2, w.n_matched.as<unsigned long long>());
    WM_HIP(ctx, hipGetLastError());
    WM_HIP(ctx, hipEventRecord(w.ev[1], st));
    WM_HIP(ctx, hipMemcpyAsync(w.h.p, w.n_matched.p, 8, hipMemcpyDeviceToHost, st));
    WM_HIP(ctx, hipStreamSynchronize(st));
    if (stats) {
        stats->n_matched = (size_t) *w.h.as<unsigned long long>();
        (void) hipEventElapsedTime(&stats->kernel_ms, w.ev[0], w.ev[1]);
    }
    if (out_mem == WM_MEM_HOST) {
        WM_TRY(copy_to_caller(ctx, idx_out, d_idx, na * 4));
        if (d2_out) WM_TRY(copy_to_caller(ctx, d2_out, d_d2, na * 4));
    }
    return WM_OK;
}
