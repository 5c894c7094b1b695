// wm_fetch.hip -- small transfers between the device and a waiting host: the fetch of a small result by one
// wavefront that copies, fences and signals (fast_fetch*), column sums delivered the same way (k_sum_fetch), the waits
// for such a flag or for slots a kernel fills (host_wait, wm_internal.hpp), the pinned scratch they land in, and the
// plain copies.  Used by every registration path, the voxel filter, the grid build and the sharding planner.
#include "wm_internal.hpp"

namespace wm {

// a plain float4 copy: what this GPU's HBM delivers to a streaming kernel (read + write).  NT:
// four loads in flight per lane, non-temporal both ways (scripts/dev/copy_probe.hip: which shape
// wins varies from box to box by ~10 %, so wm_debug_copy_bandwidth reports the best of three)
typedef float copy_f4v __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ void __launch_bounds__(256) k_copy_f4(const copy_f4v *__restrict__ a, copy_f4v *__restrict__ b, size_t n) {
    const size_t stride = (size_t) gridDim.x * 256u;
    size_t i = (size_t) blockIdx.x * 256u + threadIdx.x;
    if constexpr (NT) {
        for (; i + 3 * stride < n; i += 4 * stride) {
            copy_f4v v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(a + i + u * stride);
#pragma unroll
            for (int u = 0; u < 4; ++u) __builtin_nontemporal_store(v[u], b + i + u * stride);
        }
    }
    for (; i < n; i += stride) b[i] = a[i];
}

// Small results the host has to wait for (bounding-box / occupancy partials, the iteration
// state, a voxel count, the GICP objective's sums) are produced in DEVICE memory and then
// fetched by ONE wavefront that copies them into pinned host memory, executes a system-scope
// fence in every lane, and only then raises the completion flag the host polls.  Anything
// weaker was seen to fail a few times in a hundred runs on some machines: a flag written by a
// later kernel (or a DMA copy followed by a signalling kernel) can reach host memory BEFORE
// data written by other compute units / engines, which travel other routes through the fabric
// -- the host then reads stale partials (a bounding-box count larger than the cloud, a stale
// voxel count) and the next kernel walks off the end of a buffer.
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
    k_fetch_signal(unsigned *dst, const unsigned *src, unsigned words, unsigned *flag, unsigned seq) {
    if ((words & 3u) == 0 && (((size_t) dst | (size_t) src) & 15u) == 0) {
        const uint4 *s4 = (const uint4 *) src;
        uint4 *d4 = (uint4 *) dst;
        for (unsigned w = threadIdx.x; w < words / 4; w += THREADS) d4[w] = s4[w];
    } else {
        for (unsigned w = threadIdx.x; w < words; w += THREADS) dst[w] = src[w];
    }
    __threadfence_system();  // every lane: all of this wave's stores are performed system-wide
    // more than one wave (large fetches): each has fenced its own stores before it arrives here,
    // and the flag is written after all of them have
    if (THREADS > 64) __syncthreads();
    if (threadIdx.x == 0) *(volatile unsigned *) flag = seq;
}

static int wait_flag(wm_ctx *ctx, unsigned seq) {
    // host_wait's three stages; after 4 ms the runtime blocks -- which is also what reports a failed kernel
    volatile unsigned *flag = ctx->h_sig;
    return host_wait(ctx, [&] { return *flag == seq; }, std::chrono::milliseconds(4)) == kWaitFailed ? WM_ERR_HIP : WM_OK;
}

// wait until the n 16-byte slots {value, number} at `slots` (pinned memory) all carry `seq` (host_wait's three stages:
// spin, poll with yields, and after 4 ms let the runtime block -- which is also what reports a failed kernel)
int wait_slots(wm_ctx *ctx, const double *slots, int n, unsigned seq) {
    const volatile unsigned *w = reinterpret_cast<const volatile unsigned *>(slots);
    auto all_there = [&]() {
        for (int k = n - 1; k >= 0; --k)
            if (w[4 * k + 2] != seq) return false;
        return true;
    };
    const HostWait hw = host_wait(ctx, all_there, std::chrono::milliseconds(4));
    if (hw == kWaitFailed) return WM_ERR_HIP;
    if (hw == kWaitBlocked && !all_there()) {
        ctx->last_error = "the kernel ended without delivering its sums";
        return WM_ERR_HIP;
    }
    return WM_OK;
}

int fast_fetch_begin(wm_ctx *ctx, unsigned **flag, unsigned *seq) {
    if (!ctx->h_sig) {
        WM_HIP(ctx, hipHostMalloc((void **) &ctx->h_sig, 64, hipHostMallocDefault));
        *ctx->h_sig = 0;
    }
    *flag = ctx->h_sig;
    *seq = ++ctx->sig_seq;
    return WM_OK;
}

int fast_fetch_wait(wm_ctx *ctx, unsigned seq) { return wait_flag(ctx, seq); }

int fast_fetch(wm_ctx *ctx, void *dst_pinned, const void *src_dev, size_t bytes) {
    if (bytes & 3) return WM_ERR_ARG;
    if (!ctx->h_sig) {
        WM_HIP(ctx, hipHostMalloc((void **) &ctx->h_sig, 64, hipHostMallocDefault));
        *ctx->h_sig = 0;
    }
    const unsigned seq = ++ctx->sig_seq;
    if (bytes <= 4096)  // one wave: nothing to wait for but its own stores
        hipLaunchKernelGGL(k_fetch_signal<64>, dim3(1), dim3(64), 0, ctx->stream, (unsigned *) dst_pinned,
                           (const unsigned *) src_dev, (unsigned) (bytes / 4), ctx->h_sig, seq);
    else
        hipLaunchKernelGGL(k_fetch_signal<1024>, dim3(1), dim3(1024), 0, ctx->stream, (unsigned *) dst_pinned,
                           (const unsigned *) src_dev, (unsigned) (bytes / 4), ctx->h_sig, seq);
    WM_HIP(ctx, hipGetLastError());
    return wait_flag(ctx, seq);
}

// Column sums of a [rows][k] block of f64 partials (k <= 32), reduced ON THE DEVICE by one
// workgroup and delivered as k doubles: what the host needs from a GICP objective or an NDT
// derivative pass is the sum over blocks, and shipping every block's partials over PCIe to add
// them on the host cost more than the pass's own launch.  Fixed order, no atomics: thread t
// adds elements t, t + S, t + 2S, ... (S = the largest multiple of k <= 1024, so a thread stays
// in one column and a wave reads consecutive doubles), eight threads per column then add those
// partial sums group by group, one thread per column adds the eight.  The k results are written
// and fenced by lanes of wave 0, which also writes the flag (k_fetch_signal's rule).
__global__ void __launch_bounds__(1024)
    k_sum_fetch(double *dst, const double *__restrict__ src, unsigned rows, unsigned k, unsigned *flag,
                unsigned seq) {
    __shared__ double s1[1024];
    __shared__ double s2[8][32];
    const unsigned t = threadIdx.x;
    const unsigned groups = 1024u / k, stride = groups * k, total = rows * k;
    double a = 0.0;
    if (t < stride) {
        unsigned e = t;
        for (; e + 3 * stride < total; e += 4 * stride) {  // four loads in flight, added in order
            const double v0 = src[e], v1 = src[e + stride], v2 = src[e + 2 * stride], v3 = src[e + 3 * stride];
            a += v0;
            a += v1;
            a += v2;
            a += v3;
        }
        for (; e < total; e += stride) a += src[e];
    }
    s1[t] = a;
    __syncthreads();
    if (t < 8 * k) {
        const unsigned c = t % k, g = t / k;
        double b = 0.0;
        for (unsigned gg = g; gg < groups; gg += 8) b += s1[gg * k + c];
        s2[g][c] = b;
    }
    __syncthreads();
    if (t < k) {
        double r = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) r += s2[g][t];
        dst[t] = r;
    }
    if (t < 64 && flag) {
        __threadfence_system();
        if (t == 0) *(volatile unsigned *) flag = seq;
    }
}

int fast_fetch_sum(wm_ctx *ctx, double *dst_pinned, const double *src_dev, unsigned rows, unsigned k) {
    if (k < 1 || k > 32 || rows < 1) return WM_ERR_ARG;
    if (!ctx->h_sig) {
        WM_HIP(ctx, hipHostMalloc((void **) &ctx->h_sig, 64, hipHostMallocDefault));
        *ctx->h_sig = 0;
    }
    const unsigned seq = ++ctx->sig_seq;
    hipLaunchKernelGGL(k_sum_fetch, dim3(1), dim3(1024), 0, ctx->stream, dst_pinned, src_dev, rows, k,
                       ctx->h_sig, seq);
    WM_HIP(ctx, hipGetLastError());
    return wait_flag(ctx, seq);
}

int sum_to_device(wm_ctx *ctx, double *dst_dev, const double *src_dev, unsigned rows, unsigned k) {
    if (k < 1 || k > 32 || rows < 1) return WM_ERR_ARG;
    hipLaunchKernelGGL(k_sum_fetch, dim3(1), dim3(1024), 0, ctx->stream, dst_dev, src_dev, rows, k,
                       (unsigned *) nullptr, 0u);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

int sync_sleeping(wm_ctx *ctx) {
    // an event behind what is queued, looked at every ~50 us between short sleeps: a few per cent of a core
    // per waiting thread, and the wait ends within ~0.1 ms of the work (a BLOCKING event synchronise -- the
    // runtime's interrupt path -- was seen to add up to a millisecond per wait: 59 000 -> 48 500 pairs/s for a
    // single context's 256-pair batches)
    if (!ctx->ev_block && hipEventCreateWithFlags(&ctx->ev_block, hipEventDisableTiming) != hipSuccess) {
        (void) hipGetLastError();
        ctx->ev_block = nullptr;
        WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WM_OK;
    }
    WM_HIP(ctx, hipEventRecord(ctx->ev_block, ctx->stream));
    for (;;) {
        const hipError_t e = hipEventQuery(ctx->ev_block);
        if (e == hipSuccess) return WM_OK;
        if (e != hipErrorNotReady) WM_HIP(ctx, e);
        std::this_thread::sleep_for(std::chrono::microseconds(40));
    }
}

int copy_to_caller(wm_ctx *ctx, void *dst, const void *src_dev, size_t bytes) {
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) WM_HIP(ctx, hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost));
    return WM_OK;
}

void *pinned_scratch(wm_ctx *ctx, size_t bytes) {
    if (bytes < (64u << 10)) bytes = 64u << 10;
    if (ctx->h_scratch_bytes < bytes) {
        if (ctx->h_scratch) {
            (void) hipStreamSynchronize(ctx->stream);
            (void) hipHostFree(ctx->h_scratch);
        }
        ctx->h_scratch = nullptr;
        ctx->h_scratch_bytes = 0;
        if (hipHostMalloc(&ctx->h_scratch, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
        ctx->h_scratch_bytes = bytes;
    }
    return ctx->h_scratch;
}

}  // namespace wm

using namespace wm;

extern "C" {

int wm_debug_copy_bandwidth(wm_ctx *ctx, size_t bytes, int reps, double *gb_per_s) {
    if (!ctx || !gb_per_s || bytes < (1u << 20) || reps < 1) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = bytes / sizeof(float4);
    float4 *a = nullptr, *b = nullptr;
    WM_HIP(ctx, hipMalloc((void **) &a, n * sizeof(float4)));
    if (hipMalloc((void **) &b, n * sizeof(float4)) != hipSuccess) {
        (void) hipFree(a);
        ctx->last_error = "wm_debug_copy_bandwidth: hipMalloc failed";
        return WM_ERR_NOMEM;
    }
    (void) hipMemsetAsync(a, 0x3c, n * sizeof(float4), ctx->stream);
    const copy_f4v *ca = reinterpret_cast<const copy_f4v *>(a);
    copy_f4v *cb = reinterpret_cast<copy_f4v *>(b);
    float ms = 0;
    hipError_t e = hipSuccess;
    for (int shape = 0; shape < 3; ++shape) {
        const unsigned blocks = shape == 0 ? 1024u : (shape == 1 ? 65536u : 16384u);
        for (int r = -2; r < reps; ++r) {  // two warm-up launches
            if (r == 0) (void) hipEventRecord(ctx->ev_a, ctx->stream);
            if (shape == 2) hipLaunchKernelGGL(k_copy_f4<true>, dim3(blocks), dim3(256), 0, ctx->stream, ca, cb, n);
            else hipLaunchKernelGGL(k_copy_f4<false>, dim3(blocks), dim3(256), 0, ctx->stream, ca, cb, n);
        }
        (void) hipEventRecord(ctx->ev_b, ctx->stream);
        e = hipEventSynchronize(ctx->ev_b);
        float t = 0;
        (void) hipEventElapsedTime(&t, ctx->ev_a, ctx->ev_b);
        if (e != hipSuccess) break;
        if (shape == 0 || (t > 0 && t < ms)) ms = t;
    }
    (void) hipFree(a);
    (void) hipFree(b);
    WM_HIP(ctx, e);
    *gb_per_s = ms > 0 ? 2.0 * (double) (n * sizeof(float4)) * reps / (ms * 1e-3) / 1e9 : 0.0;
    return WM_OK;
}

}  // extern "C"
