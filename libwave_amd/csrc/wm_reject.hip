// wm_reject.hip -- correspondence rejection between an ICP iteration's search and its step (wm_icp_params.reject):
// pcl::registration::CorrespondenceRejectorTrimmed and CorrespondenceRejectorMedianDistance as
// pcl::IterativeClosestPoint applies ONE of them per iteration (the contract: wavematch.h, WM_REJECT_*).
//   k_reject_hist<PASS>  the exact order statistic of the matched pairs' squared distances, on the device: a radix
//                        select over the bit pattern of d2 (a non-negative float orders as its unsigned bits; bit 31 is
//                        0) in three histogram passes -- bits 30-20, 19-9, 8-0.  A pass reads the 8-byte keys only
//                        (low word: matched or not; high word: d2), counts the digit of the keys that carry the prefix
//                        found so far -- integers: LDS atomics, one global integer add per occupied bin and workgroup,
//                        exact in any order -- and its LAST workgroup finds the bin that holds the rank, for the next
//                        pass.  The matched count n is only known on the device: the last workgroup of pass 0 forms the
//                        rule's rank from it, in double, as the contract writes it; the last of pass 2 the threshold.
//   k_reject_mark        behind a loop's last iteration: a rejected key loses its index (the context's correspondences
//                        are PCL's correspondences_, the kept pairs); the record goes into the iteration state.
// The filter itself is k_icp_stats / k_plane_stats with the threshold's address (wm_icp.hip, wm_plane.hip); the loop
// that launches all of it is icp_run_loop's.  Every kernel here returns on st->done, so that behind the last executed
// iteration the record on the device is still that iteration's.
#include "wm_internal.hpp"
#include "wm_wave.hpp"

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <new>

namespace wm {

constexpr int kRjBins = 2048;    // 11 bits per pass (the last pass: 9 bits, 512 bins)
constexpr int kRjUnroll = 4;     // keys per thread and trip, every load issued before the first use
constexpr int kRjMaxBlocks = 1024;
constexpr int kRjAllKept = 0x7F7FFFFF;            // FLT_MAX: no finite d2 is above it
constexpr int kRjNoneKept = (int) 0xBF800000u;    // -1.0f: as a signed word below every d2

struct RejectDev {
    unsigned hist[3][kRjBins];  // all zero between passes (a pass's last workgroup puts the zeros back)
    unsigned ticket[4];         // workgroups of a pass that have added their counts; zero between passes
    unsigned prefix;            // the bits of the wanted element found so far
    unsigned rank;              // its 0-based rank among the keys that carry the prefix
    unsigned skip;              // the rule needed no element (nothing matched, everything kept, nothing kept)
    unsigned n_matched;         // matched keys of this iteration
    int thr_bits;               // the threshold: kept iff (int) bits(d2) <= thr_bits
    unsigned elem_bits;         // the selected element itself (the median before its factor)
    unsigned pad[2];
};

__device__ __forceinline__ unsigned rj_shift(int pass) { return pass == 0 ? 20u : (pass == 1 ? 9u : 0u); }
__device__ __forceinline__ unsigned rj_mask(int pass) { return pass == 2 ? 0x1FFu : 0x7FFu; }

// one count per active lane into h[digit]: the lanes of a wave that share a digit are found by matching it bit by bit
// (ballots), the lowest of them adds their number -- late in a registration most d2 share a few exponents, and 64
// same-address LDS atomics of a wave would retire one after the other
template <int BITS>
__device__ __forceinline__ void rj_wave_add(unsigned *h, unsigned digit, bool act) {
    unsigned long long m = __ballot(act);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long bb = __ballot(act && bit);
        m &= bit ? bb : ~bb;
    }
    if (act) {
        const unsigned lane = threadIdx.x & 63u;
        if ((m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&h[digit], (unsigned) __popcll(m));
    }
}

// the largest float whose double value does not exceed x (x >= 0; beyond FLT_MAX: FLT_MAX), as its bit pattern: a
// bisection over the patterns, which order as the values do -- float -> double is exact, nothing is rounded
__device__ inline unsigned rj_float_below(double x) {
    if (!(x < (double) FLT_MAX)) return (unsigned) kRjAllKept;
    unsigned lo = 0u, hi = (unsigned) kRjAllKept;  // (double) lo <= x < (double) hi
    while (hi - lo > 1u) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if ((double) __uint_as_float(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// rule: WM_REJECT_TRIMMED / WM_REJECT_MEDIAN, or -1: the element of rank `rank_in` (wm_debug_rank_select)
template <int PASS>
__global__ void __launch_bounds__(kBlock)
    k_reject_hist(const unsigned long long *__restrict__ keys, unsigned n, const IcpDevState *__restrict__ st, RejectDev *rd,
                  int rule, double ratio, double factor, unsigned min_corr, unsigned rank_in) {
    if (st->done) return;
    if (PASS > 0 && rd->skip) return;  // (written by pass 0's launch: uniform over this one)
    constexpr int kBins = PASS == 2 ? 512 : kRjBins;
    constexpr int kBits = PASS == 2 ? 9 : 11;
    __shared__ unsigned h[kBins];
    __shared__ unsigned s_last, s_wave[kBlock / 64], s_bin, s_rem;
    for (unsigned b = threadIdx.x; b < (unsigned) kBins; b += kBlock) h[b] = 0u;
    const unsigned prefix = PASS > 0 ? rd->prefix : 0u;
    const unsigned pshift = PASS == 1 ? 20u : 9u;  // (PASS 1: the keys whose bits 30-20 match; PASS 2: bits 30-9)
    __syncthreads();
    const unsigned stride = gridDim.x * kBlock;
    for (unsigned i0 = blockIdx.x * kBlock + threadIdx.x; i0 - threadIdx.x < n; i0 += kRjUnroll * stride) {
        // (the trip count is uniform over the workgroup -- i0 - threadIdx.x is --: every lane reaches the ballots)
        unsigned long long kv[kRjUnroll];
#pragma unroll
        for (int u = 0; u < kRjUnroll; ++u) {
            const unsigned i = i0 + u * stride;
            kv[u] = i < n && i >= i0 ? keys[i] : ~0ull;  // (i >= i0: no wrap of the index near 2^32)
        }
#pragma unroll
        for (int u = 0; u < kRjUnroll; ++u) {
            const unsigned bits = (unsigned) (kv[u] >> 32);
            bool act = (unsigned) kv[u] != kNoIdx;
            if (PASS > 0) act = act && (bits >> pshift) == (prefix >> pshift);
            rj_wave_add<kBits>(h, (bits >> rj_shift(PASS)) & rj_mask(PASS), act);
        }
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < (unsigned) kBins; b += kBlock) {
        const unsigned c = h[b];
        if (c) (void) __hip_atomic_fetch_add(&rd->hist[PASS][b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the last workgroup to have added its counts resolves the pass (the ticket recipe of the NDT passes, wm_ndt.hip:
    // every wave waits for its own adds, one relaxed agent-scope ticket, the last arrival reads at agent scope)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&rd->ticket[PASS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    // thread t: bins [t * kPer, t * kPer + kPer), read and set back to zero for the next iteration
    constexpr int kPer = kBins / kBlock;
    unsigned c[kPer], mine = 0u;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        unsigned *w = &rd->hist[PASS][threadIdx.x * kPer + j];
        c[j] = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine += c[j];
    }
    // exclusive sum of `mine` over the workgroup's threads
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned incl = wave_incl_scan(mine, lane);
    if (lane == 63u) s_wave[wave] = incl;
    if (threadIdx.x == 0) s_bin = 0xFFFFFFFFu;
    __syncthreads();
    unsigned before = incl - mine, total = 0u;
    for (unsigned w = 0; w < (unsigned) (kBlock / 64); ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    // the rank looked for: pass 0 forms it from the matched count (its histogram's total), the others were handed it
    unsigned rank = PASS > 0 ? rd->rank : 0u;
    bool skip = false;
    int skip_thr = kRjAllKept;
    if (PASS == 0) {
        const unsigned nm = total;
        if (rule == WM_REJECT_TRIMMED) {
            const unsigned fl = (unsigned) floor(ratio * (double) nm);
            const unsigned k = fl > min_corr ? fl : min_corr;
            if (k >= nm) skip = true;                       // nothing is rejected (nothing matched included)
            else if (k == 0u) skip = true, skip_thr = kRjNoneKept;  // everything is
            else rank = k - 1u;                             // the k-th smallest, 1-based
        } else if (rule == WM_REJECT_MEDIAN) {
            if (nm == 0u) skip = true;
            else rank = nm / 2u;
        } else {
            rank = rank_in;
            if (rank >= nm) skip = true;
        }
    }
    if (!skip && rank >= before && rank - before < mine) {  // exactly one thread: the counts' sum is above the rank
        unsigned run = before;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (rank >= run && rank - run < c[j]) {
                s_bin = threadIdx.x * kPer + j;
                s_rem = rank - run;
            }
            run += c[j];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&rd->ticket[PASS], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (PASS == 0) {
            rd->n_matched = total;
            rd->skip = skip ? 1u : 0u;
            if (skip) {
                rd->thr_bits = skip_thr;
                rd->elem_bits = 0u;
            }
        }
        if (!skip) {
            // (s_bin stays 0xFFFFFFFF only if the counts changed under the pass: then nothing is kept -- loud, not wrong)
            const unsigned found = s_bin == 0xFFFFFFFFu ? 0u : s_bin;
            const unsigned pre = prefix | (found << rj_shift(PASS));
            rd->prefix = pre;
            rd->rank = s_rem;
            if (PASS == 2) {
                rd->elem_bits = pre;
                int thr = (int) pre;
                if (rule == WM_REJECT_MEDIAN) thr = (int) rj_float_below((double) __uint_as_float(pre) * factor);
                if (s_bin == 0xFFFFFFFFu) thr = kRjNoneKept;
                rd->thr_bits = thr;
            }
        }
    }
}

// behind the last iteration of a rejecting loop: the keys become PCL's correspondences_ (a rejected pair loses its
// index, its d2 stays), the last executed iteration's record goes into the state the host fetches
__global__ void __launch_bounds__(kBlock)
    k_reject_mark(unsigned long long *__restrict__ keys, unsigned n, IcpDevState *st, const RejectDev *__restrict__ rd) {
    const int thr = rd->thr_bits;
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0u) {
        st->n_matched = (int) rd->n_matched;
        st->reject_bits = thr;
    }
    if (i >= n) return;
    const unsigned long long key = keys[i];
    if ((unsigned) key != kNoIdx && (int) (unsigned) (key >> 32) > thr) keys[i] = key | 0xFFFFFFFFull;
}

// developer entry points: floats -> keys that all count as matched; the kept mask in the caller's order
__global__ void __launch_bounds__(kBlock)
    k_reject_keys_from_floats(const unsigned *__restrict__ bits, unsigned n, unsigned long long *__restrict__ keys) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) keys[i] = (unsigned long long) bits[i] << 32;
}

__global__ void __launch_bounds__(kBlock)
    k_reject_mask(const float4 *__restrict__ src, unsigned n, unsigned n_out, const unsigned long long *__restrict__ keys,
                  const int *__restrict__ rej, unsigned char *__restrict__ mask) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int thr = rej ? *rej : 0x7FFFFFFF;
    const unsigned orig = __float_as_uint(src[i].w);
    const unsigned long long key = keys[i];
    if (orig < n_out) mask[orig] = (unsigned) key != kNoIdx && (int) (unsigned) (key >> 32) <= thr ? 1 : 0;
}

// ------------------------------------------------------------------ host
bool reject_params_ok(int reject, double ratio, double factor, int min_corr) {
    if (reject != WM_REJECT_NONE && reject != WM_REJECT_TRIMMED && reject != WM_REJECT_MEDIAN) return false;
    if (!(ratio >= 0.0 && ratio <= 1.0)) return false;           // (NaN fails both)
    if (!(factor >= 0.0 && factor <= DBL_MAX)) return false;     // finite, >= 0
    return min_corr >= 0;
}

int reject_ready(wm_ctx *ctx) {
    WM_HIP(ctx, ctx->reject_buf.reserve(sizeof(RejectDev)));
    WM_HIP(ctx, hipMemsetAsync(ctx->reject_buf.p, 0, sizeof(RejectDev), ctx->stream));
    return WM_OK;
}

const int *reject_threshold(const wm_ctx *ctx) { return &ctx->reject_buf.as<RejectDev>()->thr_bits; }

int launch_reject_select(wm_ctx *ctx, const unsigned long long *keys, unsigned n, int rule, double ratio, double factor,
                         unsigned min_corr, unsigned rank) {
    if (!ctx->reject_buf.p) return WM_ERR_STATE;
    unsigned blocks = (n + kBlock * kRjUnroll - 1u) / (kBlock * kRjUnroll);
    if (blocks > (unsigned) kRjMaxBlocks) blocks = kRjMaxBlocks;
    if (blocks < 1u) blocks = 1u;
    const IcpDevState *st = ctx->d_state.as<IcpDevState>();
    RejectDev *rd = ctx->reject_buf.as<RejectDev>();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reject_hist<0>), dim3(blocks), dim3(kBlock), 0, ctx->stream, keys, n, st, rd, rule, ratio,
                       factor, min_corr, rank);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reject_hist<1>), dim3(blocks), dim3(kBlock), 0, ctx->stream, keys, n, st, rd, rule, ratio,
                       factor, min_corr, rank);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reject_hist<2>), dim3(blocks), dim3(kBlock), 0, ctx->stream, keys, n, st, rd, rule, ratio,
                       factor, min_corr, rank);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

int launch_reject_mark(wm_ctx *ctx) {
    const unsigned n = (unsigned) ctx->n_src;
    hipLaunchKernelGGL(k_reject_mark, dim3(n > 0 ? (n + kBlock - 1) / kBlock : 1u), dim3(kBlock), 0, ctx->stream,
                       ctx->keys.as<unsigned long long>(), n, ctx->d_state.as<IcpDevState>(), ctx->reject_buf.as<RejectDev>());
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

static int fetch_record(wm_ctx *ctx, RejectDev *tail_host) {  // everything behind the histograms
    constexpr size_t off = offsetof(RejectDev, ticket);
    WM_HIP(ctx, hipMemcpyAsync(reinterpret_cast<unsigned char *>(tail_host) + off, ctx->reject_buf.as<unsigned char>() + off,
                               sizeof(RejectDev) - off, hipMemcpyDeviceToHost, ctx->stream));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

}  // namespace wm

using namespace wm;

extern "C" {

int wm_debug_rank_select(wm_ctx *ctx, const float *vals, size_t n, size_t rank, float *out) {
    if (!ctx || !vals || !out || n == 0 || n > 0x7FFFFFF0u || rank >= n) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_HIP(ctx, ctx->reject_tmp.reserve(n * (sizeof(unsigned long long) + sizeof(unsigned))));
    WM_HIP(ctx, ctx->d_state.reserve(sizeof(IcpDevState)));
    unsigned long long *keys = ctx->reject_tmp.as<unsigned long long>();
    unsigned *bits = reinterpret_cast<unsigned *>(keys + n);
    WM_HIP(ctx, hipMemcpyAsync(bits, vals, n * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    WM_HIP(ctx, hipMemsetAsync(ctx->d_state.p, 0, sizeof(IcpDevState), ctx->stream));  // (done == 0)
    hipLaunchKernelGGL(k_reject_keys_from_floats, dim3((unsigned) ((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       bits, (unsigned) n, keys);
    WM_TRY(reject_ready(ctx));
    WM_TRY(launch_reject_select(ctx, keys, (unsigned) n, -1, 0.0, 0.0, 0u, (unsigned) rank));
    RejectDev *h = new (std::nothrow) RejectDev();
    if (!h) return WM_ERR_NOMEM;
    const int rc = fetch_record(ctx, h);
    const bool ok = rc == WM_OK && !h->skip && h->n_matched == (unsigned) n;
    unsigned eb = h->elem_bits;
    delete h;
    if (rc != WM_OK) return rc;
    if (!ok) {
        ctx->last_error = "rank select: the kernels' count of the values is not n";
        return WM_ERR_STATE;
    }
    memcpy(out, &eb, sizeof(float));
    return WM_OK;
}

int wm_icp_reject(wm_ctx *ctx, const double T[16], int mode, int reject, double ratio, double factor, int min_corr,
                  wm_icp_reject_result *res, unsigned char *kept_out, double stats_out[WM_STATS_LEN]) {
    if (!ctx || !T || !res || (mode != WM_ICP_SVD && mode != WM_ICP_GN6 && mode != WM_ICP_PLANE)) return WM_ERR_ARG;
    if (!reject_params_ok(reject, ratio, factor, min_corr)) return WM_ERR_ARG;
    if (!ctx->have_corr) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(prepare_work(ctx));
    wm_icp_params p;
    wm_icp_default_params(&p);
    p.mode = mode;
    init_state(ctx->h_state, T, &p, DBL_MAX);
    WM_TRY(upload_state(ctx));
    WM_TRY(reject_ready(ctx));
    const unsigned n = (unsigned) ctx->n_src;
    const int *rej = nullptr;
    if (reject != WM_REJECT_NONE) {
        WM_TRY(launch_reject_select(ctx, ctx->keys.as<unsigned long long>(), n, reject, ratio, factor, (unsigned) min_corr, 0u));
        rej = reject_threshold(ctx);
    }
    if (mode == WM_ICP_PLANE) {
        WM_TRY(plane_target_normals(ctx, ctx->plane_nrm_valid ? ctx->plane_nrm_k : 0));
        WM_TRY(plane_bins_ready(ctx));
        WM_TRY(launch_plane_stats(ctx, rej));
        WM_TRY(launch_plane_solve(ctx, nullptr, 0, 0));
    } else {
        WM_TRY(launch_stats(ctx, mode, rej));
        WM_TRY(launch_sum_rows(ctx));
    }
    const size_t n_in = ctx->n_src_input;
    if (kept_out && n_in > 0) {
        WM_HIP(ctx, ctx->reject_tmp.reserve(n_in));
        WM_HIP(ctx, hipMemsetAsync(ctx->reject_tmp.p, 0, n_in, ctx->stream));  // (dropped, non-finite points: not kept)
        if (n > 0) {
            hipLaunchKernelGGL(k_reject_mask, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream,
                               ctx->src_sorted.as<float4>(), n, (unsigned) n_in, ctx->keys.as<unsigned long long>(), rej,
                               ctx->reject_tmp.as<unsigned char>());
            WM_HIP(ctx, hipGetLastError());
        }
    }
    WM_HIP(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state.p, sizeof(IcpDevState), hipMemcpyDeviceToHost, ctx->stream));
    RejectDev *h = new (std::nothrow) RejectDev();
    if (!h) return WM_ERR_NOMEM;
    memset(h, 0, sizeof(*h));
    const int rc = fetch_record(ctx, h);  // (waits for the stream: the state has arrived too)
    const RejectDev rec_tail = *h;
    delete h;
    if (rc != WM_OK) return rc;
    const double *st = ctx->h_state->stats;
    res->n_kept = (int) st[0];  // ([0] is the pairs' count in every layout)
    if (reject == WM_REJECT_NONE) {
        res->n_matched = res->n_kept;
        res->threshold_d2 = FLT_MAX;
        res->all_kept = 1;
    } else {
        res->n_matched = (int) rec_tail.n_matched;
        memcpy(&res->threshold_d2, &rec_tail.thr_bits, sizeof(float));
        res->all_kept = rec_tail.thr_bits == kRjAllKept ? 1 : 0;
    }
    if (stats_out) memcpy(stats_out, st, sizeof(double) * WM_STATS_LEN);
    if (kept_out && n_in > 0) WM_TRY(copy_to_caller(ctx, kept_out, ctx->reject_tmp.p, n_in));
    return WM_OK;
}

}  // extern "C"
