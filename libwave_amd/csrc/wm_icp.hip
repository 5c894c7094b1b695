// wm_icp.hip -- the ICP iteration on the device and the registration driver around it: the statistics and solve
// kernels with their launchers, the iteration state's init / upload / download, the loop that runs ahead of the
// device (icp_run_loop and its steps), and the C ABI of a registration -- wm_icp_align, wm_icp_match, the
// correspondence and statistics queries, the sharded stepping API and the host-only state machine.
// (The context and its clouds: wm_ctx.hip; the small transfers and waits: wm_fetch.hip; developer output: wm_debug.hip.)
//
// One iteration of pcl::IterativeClosestPoint::computeTransformation
// [PCL registration/impl/icp.hpp], as driven by libwave's ICPMatcher::match()
// (wave_matching/src/icp.cpp:95,116,126), is three kernel classes:
//   1. correspondence search (wm_nn.hip)                 -> 8-byte key per source point
//   2. k_icp_stats: streaming reduction of the matched pairs to 17 doubles
//      per workgroup (n, sum p, sum q, sum q p^T, sum d2  |  GN: n, sum p,
//      A^T A, J^T r, sum d2)
//   3. k_reduce_solve: fixed-order sum of the partials, the 3x3 SVD (Umeyama) or
//      6x6 solve (Gauss-Newton), T <- T_k T, and PCL's DefaultConvergenceCriteria,
//      all by one workgroup, so the whole registration runs with the host out of
//      the loop.  In the multi-GPU path the 32-double statistics block is what
//      the RCCL all-reduce carries between (2) and (3).
#include "wm_internal.hpp"
#include "wm_icp_step.hpp"
#include "wm_pair_terms.hpp"
#include "wm_bins.hpp"
#include "wm_xchg.hpp"

#include <chrono>
#include <utility>
#include <vector>

#include <float.h>
#include <math.h>
#include <string.h>

#include <new>

namespace wm {

constexpr int kMaxStatBlocks = 256;
constexpr int kStatUnroll = 4;  // points per thread per trip of the statistics kernel

// Per-workgroup partial sums, written as partials[block][kAcc].
template <int MODE>
__global__ void __launch_bounds__(kBlock)
    k_icp_stats(const float4 *__restrict__ src, unsigned n,
                const unsigned long long *__restrict__ keys, const float4 *__restrict__ tgt,
                const IcpDevState *__restrict__ st, double *__restrict__ partials, const int *__restrict__ rej) {
    if (st->done) return;
    // correspondence rejection (wm_reject.hip): a matched pair counts iff its d2's bit pattern is <= the threshold's
    // (signed: "reject everything" is a negative one); no rejection: no d2 is above INT_MAX
    const int rej_thr = rej ? *rej : 0x7FFFFFFF;
    double a[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) a[k] = 0.0;
    const bool slab_on = st->slab_on != 0;
    const float slab_lo = st->slab_lo, slab_hi = st->slab_hi;
    // kStatUnroll points per trip: all their loads are issued before the first use, so a wave keeps
    // ~10 KB in flight (the kernel is a pure HBM/L2 stream); accumulation order is unchanged
    const unsigned stride = gridDim.x * kBlock;
    for (unsigned i0 = blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kStatUnroll * stride) {
        float4 p4v[kStatUnroll], q4v[kStatUnroll];
        unsigned long long keyv[kStatUnroll];
#pragma unroll
        for (int u = 0; u < kStatUnroll; ++u) {
            const unsigned i = i0 + u * stride;
            const unsigned ic = i < n ? i : i0;
            p4v[u] = src[ic];
            keyv[u] = keys[ic];
            q4v[u] = tgt[ic];  // match coordinates, written by the search (coalesced)
        }
#pragma unroll
        for (int u = 0; u < kStatUnroll; ++u) {
            if (i0 + u * stride >= n) break;
            float fx, fy, fz;
            xform_pcl(st->Tf, p4v[u].x, p4v[u].y, p4v[u].z, fx, fy, fz);
            // sharded registration: the same ownership test as the search kernel
            if (slab_on && !(fx >= slab_lo && fx < slab_hi)) continue;
            a[17] += 1.0;
            const unsigned long long key = keyv[u];
            if ((unsigned) key == kNoIdx) continue;
            if ((int) (unsigned) (key >> 32) > rej_thr) continue;  // rejected
            icp_pair_terms<MODE>(fx, fy, fz, q4v[u].x, q4v[u].y, q4v[u].z, __uint_as_float((unsigned) (key >> 32)),
                                 [&](int k, double term) { a[k] += term; });
        }
    }
    // wave reduction (fixed xor-tree order), then across the 4 waves through LDS
#pragma unroll
    for (int k = 0; k < kAcc; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_down(a[k], off);
    __shared__ double lds[kBlock / 64][kAcc];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < kAcc; ++k) lds[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x < kAcc) {
        double s = 0;
        for (int w = 0; w < kBlock / 64; ++w) s += lds[w][threadIdx.x];
        partials[(size_t) blockIdx.x * kAcc + threadIdx.x] = s;
    }
}

// Pre-reduction for very many partial rows (fused statistics of clouds beyond ~1M points per GPU,
// or one-wave workgroups): block b adds rows [128 b, 128 b + 128) in a fixed order -> out row b.
constexpr int kPreRows = 128;
__global__ void __launch_bounds__(kBlock)
    k_reduce_rows(const double *__restrict__ partials, int rows, const IcpDevState *__restrict__ st,
                  double *__restrict__ out) {
    if (st->done) return;
    constexpr int kLanes = kBlock / kAcc;  // 14 row-lanes x kAcc components
    __shared__ double lds[kLanes][kAcc];
    const int c = threadIdx.x % kAcc, r = threadIdx.x / kAcc;
    const int r0 = blockIdx.x * kPreRows, r1 = min(r0 + kPreRows, rows);
    if (r < kLanes) {
        double v[(kPreRows + kLanes - 1) / kLanes];
        int k = 0;
#pragma unroll
        for (int b = r0 + r, u = 0; u < (kPreRows + kLanes - 1) / kLanes; b += kLanes, ++u, ++k)
            v[u] = b < r1 ? partials[(size_t) b * kAcc + c] : 0.0;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < (kPreRows + kLanes - 1) / kLanes; ++u) s += v[u];
        lds[r][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < kAcc) {
        double t = 0.0;
#pragma unroll
        for (int l = 0; l < kLanes; ++l) t += lds[l][threadIdx.x];
        out[(size_t) blockIdx.x * kAcc + threadIdx.x] = t;
    }
}

// The iteration's solve from the BINS the search kernel's waves added their sums into (wm_bins.hpp): the unsharded
// loop's replacement for k_reduce_rows + k_reduce_solve<3>.  One workgroup: thread (g, j) adds word j (limb, component)
// of bins g, g + kGroups, ... -- integers: exact in any order --, the kGroups partial totals meet in LDS, one thread per
// component turns its three limb totals back into a double (bins_value), thread 0 runs the solve, PCL's stopping rules
// and publishes the record exactly as k_reduce_solve does; the words read are set back to zero for the next iteration.
__global__ void __launch_bounds__(kBlock)
    k_bins_solve(long long *__restrict__ bins, IcpDevState *st, unsigned long long *pub, int pub_slots) {
    __shared__ IcpDevState s_st;
    __shared__ BinsLds s_b;
    const unsigned long long t_start = clock64();
    static_assert(sizeof(IcpDevState) % 4 == 0, "word-wise staging");
    constexpr unsigned kWords = sizeof(IcpDevState) / 4;
    constexpr unsigned kStage = (kWords + kBlock - 1) / kBlock;
    unsigned stage[kStage];
#pragma unroll
    for (unsigned k = 0; k < kStage; ++k) {  // (the state's loads and the bins' in ONE round trip)
        const unsigned w = threadIdx.x + k * kBlock;
        stage[k] = w < kWords ? reinterpret_cast<const unsigned *>(st)[w] : 0u;
    }
    bins_collect<kBlock>(bins, s_b);
#pragma unroll
    for (unsigned k = 0; k < kStage; ++k) {
        const unsigned w = threadIdx.x + k * kBlock;
        if (w < kWords) reinterpret_cast<unsigned *>(&s_st)[w] = stage[k];
    }
    __syncthreads();
    if (s_st.done) return;  // (uniform; a launch queued behind a `done`: the bins were all zero and stay so)
    if (threadIdx.x == 0) {
        s_st.dbg[0] = t_start;
        s_st.dbg[1] = clock64();
        double a[kAcc], ex[kStatsLen];
#pragma unroll
        for (int k = 0; k < kAcc; ++k) a[k] = s_b.poison ? 0.0 : s_b.tot[k];  // (poisoned: "no correspondences", icp_apply_stats)
        expand_stats(s_st.mode, a, ex, s_st.changed_mask);
        s_st.local_handled = ex[kStatsLen - 1];
#pragma unroll
        for (int k = 0; k < kStatsLen; ++k) s_st.stats[k] = ex[k];
        s_st.dbg[2] = clock64();
        icp_apply_stats(&s_st, ex, (long long) s_b.tot[kAcc]);
        publish_step(&s_st, pub, pub_slots);
        s_st.dbg[3] = clock64();
    }
    __syncthreads();
    for (unsigned w = threadIdx.x; w < kWords; w += kBlock)
        reinterpret_cast<unsigned *>(st)[w] = reinterpret_cast<const unsigned *>(&s_st)[w];
}

// PHASE 1: sum partials -> st->stats.   PHASE 2: solve + criteria from st->stats.
// Single GPU launches <1|2>; the sharded path launches <1>, all-reduces
// st->stats over RCCL, then launches <2>.
// THREADS = 256 for the few rows of k_icp_stats, 1024 for the thousands of rows the fused search
// kernel leaves (one row per workgroup).
// PHASES == 7 (sharded loop, mailboxes available): 1, then the exchange of the block with the other ranks INSIDE this
// kernel (wm_xchg.hpp), then 2 -- one launch per iteration where <1>, ncclAllReduce, <2> are three.
template <int PHASES, int THREADS>
__global__ void __launch_bounds__(THREADS)
    k_reduce_solve(const double *__restrict__ partials, int nblocks, IcpDevState *st,
                   double *stats_io, unsigned long long *pub, int pub_slots, int blk_ext, XchgDev xd, long long *bins) {
    // (bins != nullptr, phases with bit 0: this rank's sums come out of the iteration's bins -- exact integer limbs the
    // search kernel's waves added into, wm_bins.hpp -- instead of rows of partial sums: no k_reduce_rows in front)
    // (blk_ext: stats_io is the sharded loop's kBlkLen block, not a caller's WM_STATS_LEN one)
    // The solve runs in ONE lane and touches two dozen fields of the state: read from HBM one
    // dependent access at a time that is most of this kernel's ~10 us.  So the whole state is
    // staged in LDS by all threads (one round trip), worked on there, and written back whole.
    __shared__ IcpDevState s_st;
    const unsigned long long t_start = clock64();
    static_assert(sizeof(IcpDevState) % 4 == 0, "word-wise staging");
    constexpr unsigned kWords = sizeof(IcpDevState) / 4;
    // (the state's loads are issued here and land in LDS after the rows' loads have been issued
    // too: one memory round trip for both, not two)
    constexpr unsigned kStage = (kWords + THREADS - 1) / THREADS;
    unsigned stage[kStage];
#pragma unroll
    for (unsigned k = 0; k < kStage; ++k) {
        const unsigned w = threadIdx.x + k * THREADS;
        stage[k] = w < kWords ? reinterpret_cast<const unsigned *>(st)[w] : 0u;
    }
    constexpr int kRows = THREADS / kAcc;  // row-lanes x kAcc components <= THREADS threads
    constexpr int kGroups = 8;
    __shared__ double lds[kRows][kAcc];
    __shared__ double lds2[kGroups][kAcc];
    __shared__ double tot[kAcc];
    __shared__ BinsLds s_b;
    const bool from_bins = (PHASES & 1) && bins != nullptr;
    if (from_bins) {
        bins_collect<THREADS>(bins, s_b);
    } else if (PHASES & 1) {
        // thread (r, c) adds rows r, r + kRows, ... of column c: a wave reads 64 consecutive
        // doubles per load; 16 independent accumulators keep 16 loads in flight (every dependent
        // load -> add would cost a memory latency)
        const int c = threadIdx.x % kAcc, r = threadIdx.x / kAcc;
        if (r < kRows) {
            constexpr int U = 16;
            double s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = 0.0;
            for (int b = r; b < nblocks; b += U * kRows) {  // every batch: U loads, then U adds
                double v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int bb = b + u * kRows;
                    v[u] = bb < nblocks ? partials[(size_t) bb * kAcc + c] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) s[u] += v[u];
            }
#pragma unroll
            for (int w = U / 2; w > 0; w >>= 1)
#pragma unroll
                for (int u = 0; u < w; ++u) s[u] += s[u + w];
            lds[r][c] = s[0];
        }
    }
#pragma unroll
    for (unsigned k = 0; k < kStage; ++k) {
        const unsigned w = threadIdx.x + k * THREADS;
        if (w < kWords) reinterpret_cast<unsigned *>(&s_st)[w] = stage[k];
    }
    if (from_bins) {
        if (threadIdx.x < (unsigned) kAcc) tot[threadIdx.x] = s_b.poison ? 0.0 : s_b.tot[threadIdx.x];
    } else if (PHASES & 1) {
        const int c = threadIdx.x % kAcc;
        __syncthreads();
        if (threadIdx.x < kGroups * kAcc) {  // row-lanes g, g + 8, ... of column c
            const int g = threadIdx.x / kAcc;
            double t = 0.0;
            for (int sl = g; sl < kRows; sl += kGroups) t += lds[sl][c];
            lds2[g][c] = t;
        }
        __syncthreads();
        if (threadIdx.x < kAcc) {
            double t = 0.0;
#pragma unroll
            for (int g = 0; g < kGroups; ++g) t += lds2[g][threadIdx.x];
            tot[threadIdx.x] = t;
        }
    }
    __syncthreads();
    if (s_st.done) return;  // (uniform: every thread reads the staged copy)
    // the certificate kernel's 64 partial counts of searched queries: added (and zeroed) by the first
    // wave here, not one LDS round trip after the other by the lane that solves
    __shared__ unsigned s_uns;
    if (threadIdx.x < 64) {
        unsigned v = s_st.cert_unsettled[threadIdx.x];
        s_st.cert_unsettled[threadIdx.x] = 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += (unsigned) __shfl_xor((int) v, off);
        if (threadIdx.x == 0) s_uns = from_bins ? (unsigned) s_b.tot[kAcc] : v;  // (bins: the count is one of their components)
    }
    if constexpr (PHASES == 7) {
        // this rank's block -> every rank's mailbox; every rank's block -> the sum, in rank order (all threads)
        __shared__ double s_blk[kBlkLen], s_sum[kBlkLen];
        __shared__ unsigned s_half[kXMaxWorld * kXWords], s_ctl[2];
        if (threadIdx.x == 0) {
            double a[kAcc];
#pragma unroll
            for (int k = 0; k < kAcc; ++k) a[k] = tot[k];
            double ex[kStatsLen];
            expand_stats(s_st.mode, a, ex, s_st.changed_mask);
            s_st.local_handled = ex[kStatsLen - 1];
            ex[kStatsLen - 2] = s_st.stripe_finite;  // (as in <1>: summed, it is the cloud's count)
#pragma unroll
            for (int k = 0; k < kStatsLen; ++k) s_blk[k] = ex[k];
            s_blk[kStatsLen] = (double) s_uns;
            s_blk[kStatsLen + 1] = 0.0;
        }
        __syncthreads();
        // ([kStatsLen + 1]: 0 in an iteration's block, 1 in the block of a rank's COMMIT round (k_xchg_commit): a rank
        // that gave up on an earlier round is a round behind and sends its commit where the others expect an
        // iteration -- they then fail at once instead of solving from it)
        const bool arrived = xchg_allreduce<THREADS>(xd, s_blk, s_sum, s_half, s_ctl) && s_sum[kStatsLen + 1] == 0.0;
        if (threadIdx.x == 0) {
            s_st.dbg[0] = t_start;
            s_st.dbg[1] = clock64();
            if (!arrived) {  // a peer never delivered (or has given up): the registration ends here, on this rank, with an error
                s_st.xchg_failed = 1;
                s_st.done = 1;
                s_st.converged = 0;
                if (pub) __hip_atomic_store(pub, pack_done_word(1, s_st.iter), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            } else {
                double stats[kStatsLen];
#pragma unroll
                for (int k = 0; k < kStatsLen; ++k) stats[k] = s_st.stats[k] = s_sum[k];
                s_st.uns_global = 1;
                s_st.dbg[2] = clock64();
                icp_apply_stats(&s_st, stats, (long long) s_sum[kStatsLen]);
                if (stats_io)  // (the reduced block, for a caller that looks: wm_icp_shard_* / tests)
                    for (int k = 0; k < kBlkLen; ++k) stats_io[k] = s_sum[k];
                publish_step(&s_st, pub, pub_slots);
            }
            s_st.dbg[3] = clock64();
        }
    } else if (threadIdx.x == 0) {
        s_st.dbg[0] = t_start;
        s_st.dbg[1] = clock64();  // state staged, rows added
        if (PHASES & 1) {
            double a[kAcc];
#pragma unroll
            for (int k = 0; k < kAcc; ++k) a[k] = tot[k];
            double ex[kStatsLen];
            expand_stats(s_st.mode, a, ex, s_st.changed_mask);
            s_st.local_handled = ex[kStatsLen - 1];
#pragma unroll
            for (int k = 0; k < kStatsLen; ++k) s_st.stats[k] = ex[k];
            if (PHASES == 1 && stats_io) {  // the block the all-reduce works on
                ex[kStatsLen - 2] = s_st.stripe_finite;  // (a free slot of either layout: summed, it is the cloud's count)
#pragma unroll
                for (int k = 0; k < kStatsLen; ++k) stats_io[k] = ex[k];
                // (the searches this rank's certificate launch made: summed over the ranks, so that every
                // rank's host steers by the same share and picks the same kernel)
                if (blk_ext) {
                    stats_io[kStatsLen] = (double) s_uns;
                    stats_io[kStatsLen + 1] = 0.0;
                }
            }
        } else if (stats_io) {  // PHASES == 2: the all-reduced block comes in
#pragma unroll
            for (int k = 0; k < kStatsLen; ++k) s_st.stats[k] = stats_io[k];
            s_st.uns_global = blk_ext ? 1 : 0;
        }
        if (PHASES & 2) {
            double stats[kStatsLen];
#pragma unroll
            for (int k = 0; k < kStatsLen; ++k) stats[k] = s_st.stats[k];
            s_st.dbg[2] = clock64();
            const long long uns_total = (PHASES == 2 && stats_io && blk_ext) ? (long long) stats_io[kStatsLen] : (long long) s_uns;
            icp_apply_stats(&s_st, stats, uns_total);
            // what the host steers by while it runs ahead of the device (wm_icp_align): one 8-byte word in
            // pinned memory -- done flag, iterations finished, the step's size -- in ONE system-scope store
            // (pub[0]: the latest; pub[k]: iteration k's own record, so that what the host decides from
            // does not depend on when it looks)
            publish_step(&s_st, pub, pub_slots);
        }
        s_st.dbg[3] = clock64();
    }
    __syncthreads();
    for (unsigned w = threadIdx.x; w < kWords; w += THREADS)
        reinterpret_cast<unsigned *>(st)[w] = reinterpret_cast<const unsigned *>(&s_st)[w];
}

// The COMMIT round of a sharded registration whose exchange ran through the mailboxes (wm_xchg.hpp): after the last
// iteration every rank sends {did every round of mine arrive in time?, 1} and adds up what the others sent.  A rank
// whose wait timed out in the LAST executed round would otherwise end with an error while a slow peer that still got
// every block ends well -- and the next registration would find one of them in ncclAllReduce and the other polling its
// mailbox.  With this round the verdict is the same on every rank: all of them ended well, or all of them fail this
// registration (and all of them leave the mailboxes for the collective, wm_shard.hip).
__global__ void __launch_bounds__(kBlock) k_xchg_commit(IcpDevState *st, XchgDev xd) {
    __shared__ double s_blk[kBlkLen], s_sum[kBlkLen];
    __shared__ unsigned s_half[kXMaxWorld * kXWords], s_ctl[2];
    if (threadIdx.x < (unsigned) kBlkLen) s_blk[threadIdx.x] = 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        s_blk[0] = st->xchg_failed ? 0.0 : 1.0;
        s_blk[kStatsLen + 1] = 1.0;
    }
    __syncthreads();
    const bool arrived = xchg_allreduce<kBlock>(xd, s_blk, s_sum, s_half, s_ctl);
    if (threadIdx.x == 0 && (!arrived || s_sum[0] != (double) xd.world || s_sum[kStatsLen + 1] != (double) xd.world)) {
        st->xchg_failed = 1;
        st->converged = 0;
    }
}

// keys (source-sorted order) -> caller-order (match index, d2)
__global__ void __launch_bounds__(kBlock)
    k_unpack_corr(const float4 *__restrict__ src, unsigned n,
                  const unsigned long long *__restrict__ keys, int *__restrict__ match,
                  float *__restrict__ d2) {
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned orig = __float_as_uint(src[i].w);
    const unsigned long long key = keys[i];
    const unsigned idx = (unsigned) key;
    match[orig] = idx == kNoIdx ? -1 : (int) idx;
    d2[orig] = __uint_as_float((unsigned) (key >> 32));
}

// ------------------------------------------------------------------ host
static int stat_blocks(size_t n) {
    size_t b = (n + kBlock - 1) / kBlock;
    if (b > kMaxStatBlocks) b = kMaxStatBlocks;
    if (b < 1) b = 1;
    return (int) b;
}

unsigned stat_rows(const wm_ctx *ctx) { return (unsigned) stat_blocks(ctx->n_src); }

int launch_stats(wm_ctx *ctx, int mode, const int *rej) {
    const unsigned n = (unsigned) ctx->n_src;
    const int nb = stat_blocks(n);
    const IcpDevState *st = ctx->d_state.as<IcpDevState>();
    if (mode == WM_ICP_SVD)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_icp_stats<WM_ICP_SVD>), dim3(nb), dim3(kBlock), 0,
                           ctx->stream, ctx->src_sorted.as<float4>(), n,
                           ctx->keys.as<unsigned long long>(), ctx->match_pt.as<float4>(), st,
                           ctx->partials.as<double>(), rej);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_icp_stats<WM_ICP_GN6>), dim3(nb), dim3(kBlock), 0,
                           ctx->stream, ctx->src_sorted.as<float4>(), n,
                           ctx->keys.as<unsigned long long>(), ctx->match_pt.as<float4>(), st,
                           ctx->partials.as<double>(), rej);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// the iteration's bins (wm_bins.hpp): allocated, and all zero -- zeroed here when first allocated or when the last loop
// that used them did not end normally; kept at zero by k_bins_solve otherwise
int bins_ready(wm_ctx *ctx) {
    if (!ctx->bins.p || ctx->bins_dirty) {
        WM_HIP(ctx, ctx->bins.reserve(kBinWords * sizeof(long long)));
        WM_HIP(ctx, hipMemsetAsync(ctx->bins.p, 0, kBinWords * sizeof(long long), ctx->stream));
        ctx->bins_dirty = false;
    }
    return WM_OK;
}

static int launch_bins_solve(wm_ctx *ctx, unsigned long long *pub, int pub_slots) {
    hipLaunchKernelGGL(k_bins_solve, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->bins.as<long long>(),
                       ctx->d_state.as<IcpDevState>(), pub, pub_slots);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

// Sum `rows` partial rows (ctx->partials) and run the requested phases of the iteration's solve.
template <int PHASES>
static int launch_reduce_solve(wm_ctx *ctx, unsigned rows, double *stats_io, unsigned long long *pub = nullptr,
                               int pub_slots = 0, int blk_ext = 0, const XchgDev *xchg = nullptr, long long *bins = nullptr) {
    if (bins) rows = 0;  // (the sums are in the bins: nothing to pre-reduce, the small instantiation)
    const XchgDev xd = xchg ? *xchg : XchgDev{nullptr, nullptr, 0, 0, 0u};
    IcpDevState *st = ctx->d_state.as<IcpDevState>();
    const double *part = ctx->partials.as<double>();
    if (rows > 2048u) {  // one workgroup cannot add that many rows quickly: 128 rows -> 1 first
        const unsigned rows2 = (rows + kPreRows - 1) / kPreRows;
        WM_HIP(ctx, ctx->partials2.reserve((size_t) rows2 * kAcc * sizeof(double)));
        hipLaunchKernelGGL(k_reduce_rows, dim3(rows2), dim3(kBlock), 0, ctx->stream, part, (int) rows, st,
                           ctx->partials2.as<double>());
        part = ctx->partials2.as<double>();
        rows = rows2;
    }
    if (rows > 512u)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reduce_solve<PHASES, 1024>), dim3(1), dim3(1024), 0, ctx->stream,
                           part, (int) rows, st, stats_io, pub, pub_slots, blk_ext, xd, bins);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reduce_solve<PHASES, kBlock>), dim3(1), dim3(kBlock), 0, ctx->stream,
                           part, (int) rows, st, stats_io, pub, pub_slots, blk_ext, xd, bins);
    WM_HIP(ctx, hipGetLastError());
    return WM_OK;
}

int launch_sum_rows(wm_ctx *ctx) { return launch_reduce_solve<1>(ctx, stat_rows(ctx), nullptr); }

void init_state(IcpDevState *s, const double *T, const wm_icp_params *p, double prev_mse) {
    memset(s, 0, sizeof(*s));
    for (int k = 0; k < 16; ++k) s->T[k] = T[k];
    for (int k = 0; k < 12; ++k) s->Tf[k] = s->Tf_search[k] = (float) T[k];
    mat4_identity(s->Tk);
    s->prev_mse = prev_mse;
    if (p) {
        s->forced = p->force_iterations > 0;
        s->max_iter = s->forced ? p->force_iterations : p->max_iter;
        s->mode = p->mode;
        s->rot_thr = 1.0 - p->t_eps;
        s->trans_thr = p->t_eps;
        s->fit_eps = p->fit_eps;
    }
}

int upload_state(wm_ctx *ctx) {
    ctx->h_state->changed_mask = changed_mask_for((unsigned) ctx->n_src);
    WM_HIP(ctx, hipMemcpyAsync(ctx->d_state.p, ctx->h_state, sizeof(IcpDevState),
                               hipMemcpyHostToDevice, ctx->stream));
    return WM_OK;
}

static int download_state(wm_ctx *ctx) {
    return fast_fetch(ctx, ctx->h_state, ctx->d_state.p, sizeof(IcpDevState));
}

static void set_step_scale(wm_ctx *ctx) {  // centre and half diagonal of the (local) source cloud: IcpDevState::step_disp
    const Bbox &b = ctx->src_bbox;
    double d2 = 0;
    for (int k = 0; k < 3; ++k) {
        ctx->h_state->src_centre[k] = 0.5f * (b.lo[k] + b.hi[k]);
        d2 += 0.25 * ((double) b.hi[k] - b.lo[k]) * ((double) b.hi[k] - b.lo[k]);
    }
    ctx->h_state->src_radius = (float) sqrt(d2);
    if (ctx->n_src == 0 || !(ctx->h_state->src_radius == ctx->h_state->src_radius)) {
        ctx->h_state->src_radius = 0.f;
        ctx->h_state->src_centre[0] = ctx->h_state->src_centre[1] = ctx->h_state->src_centre[2] = 0.f;
    }
}

// IcpDevState -> the fields of wm_icp_stats every reader of a state fills (the loop below, wm_icp_shard_poll,
// wm_host_icp_get); what only some of them know stays with them
static void stats_from_state(const IcpDevState &s, wm_icp_stats *stats) {
    stats->converged = s.converged;
    stats->iterations = s.iter;
    stats->state = s.state;
    stats->n_corr = s.n_corr;
    stats->mse = s.mse;
    stats->prev_mse = s.prev_mse;
    stats->owned_violations = s.owned_violations;
    stats->n_matched = s.n_corr;  // (no rejection; a rejecting loop's finish() knows better)
    stats->reject_d2 = 0.f;
}

namespace {

// profile mode's events of one loop, out of the context's pool: 5 slots per launched iteration (level 1 only
// fills the first two), a pair per launch of the resident kernel among them, and the sharded loop's all-reduce
// pairs behind the iterations' 5 * max_it slots
struct IterEvents {
    wm_ctx *ctx;
    int profile, max_it;
    size_t used = 0, ar;
    std::vector<int> slot;                // the iteration's first event in the pool (-1: no launch of its own)
    std::vector<unsigned char> was_cert;  // the iteration's search was a certificate launch
    std::vector<std::pair<hipEvent_t, hipEvent_t>> late;
    hipEvent_t e0 = nullptr, e1 = nullptr, e1b = nullptr, e2 = nullptr, e3 = nullptr;  // of the current iteration

    IterEvents(wm_ctx *c, int profile_, int max_it_)
        : ctx(c), profile(profile_), max_it(max_it_), ar((size_t) 5 * (size_t) max_it_), slot((size_t) max_it_, -1) {}

    void begin_iteration(int it) {
        if (!profile) return;
        slot[(size_t) it] = (int) used;
        e0 = get_event(ctx, used++);
        e1 = get_event(ctx, used++);
        if (profile >= 2) {
            e1b = get_event(ctx, used++);
            e2 = get_event(ctx, used++);
            e3 = get_event(ctx, used++);
        } else {
            used += 3;
            (void) get_event(ctx, used - 1);
        }
    }
    void note_cert(int it) {
        if (!profile) return;
        was_cert.resize((size_t) it + 1, 0);
        was_cert[(size_t) it] = 1;
    }
    int record(hipEvent_t e) {
        if (e) WM_HIP(ctx, hipEventRecord(e, ctx->stream));
        return WM_OK;
    }
    // the durations, once the loop's last event has been waited for
    void read_back(const IcpDevState &s, bool sharded, wm_icp_stats *stats) {
        for (auto &ev : late) {
            float a = 0;
            if (ev.first && ev.second && hipEventElapsedTime(&a, ev.first, ev.second) == hipSuccess) ctx->late_ms += a;
        }
        stats->late_ms = ctx->late_ms;
        if (!profile) return;
        // iterations that ran (the rest of the last batch were no-ops)
        const int ran = s.iter + (s.state == WM_CONV_NO_CORRESPONDENCES || s.state == WM_CONV_DEGENERATE ? 1 : 0);
        for (int it = 0; it < ran && (size_t) it < slot.size(); ++it) {
            if (slot[(size_t) it] < 0 || (size_t) (slot[(size_t) it] + 4) >= used) {
                ctx->iter_nn_ms.push_back(-1.f);  // (ran inside the resident kernel: no launch of its own)
                continue;
            }
            float a = 0, a2 = 0, b = 0, c = 0;
            hipEvent_t *e = &ctx->ev_pool[(size_t) slot[(size_t) it]];
            (void) hipEventElapsedTime(&a, e[0], e[1]);
            if (profile >= 2) {
                (void) hipEventElapsedTime(&a2, e[1], e[2]);
                (void) hipEventElapsedTime(&b, e[2], e[3]);
                (void) hipEventElapsedTime(&c, e[3], e[4]);
            }
            ctx->iter_nn_ms.push_back(a);
            stats->nn_ms += a;
            if ((size_t) it < was_cert.size() && was_cert[(size_t) it]) stats->nn_cert_ms += a;
            stats->coarse_ms += a2;
            stats->stats_ms += b;
            stats->solve_ms += c;
            stats->nn_launches += 1;
        }
        if (!sharded) return;
        const int ran_ar = s.iter + (s.state == WM_CONV_NO_CORRESPONDENCES || s.state == WM_CONV_DEGENERATE ? 1 : 0);
        for (int it = 0; it < ran_ar; ++it) {
            const size_t k = (size_t) 5 * (size_t) max_it + 2 * (size_t) it;
            if (k + 1 >= ctx->ev_pool.size() || k + 1 >= ar) break;
            float a = 0;
            if (hipEventElapsedTime(&a, ctx->ev_pool[k], ctx->ev_pool[k + 1]) == hipSuccess) stats->allreduce_ms += a;
        }
    }
};

// One registration's loop: what icp_run_loop's steps share.
struct IcpLoop {
    wm_ctx *ctx;
    const wm_icp_params *p;
    const bool brute;
    const float thr;
    wm_comm *comm;
    double *blk;
    const int max_it, nb, kLag;
    // point-to-plane (wm_plane.hip): a search-only launch, the plane sums, their solve.  Always the FULL search: the
    // certificate kernel's policy is steered by counts only the fused statistics carry.
    const bool plane;
    // correspondence rejection (wm_reject.hip): a search-only launch, the select, the filtered sums, their solve.  Always
    // the FULL search, no fused sums, no bins for SVD / GN6.
    const bool reject;
    const bool slab;
    // the grid path adds its sums into bins (wm_bins.hpp) and solves from them -- k_bins_solve, or, sharded, the
    // k_reduce_solve that carries the exchange: no k_reduce_rows, no rows of partial sums
    const bool use_bins;
    const float cert_thr;
    XchgDev xchg{nullptr, nullptr, 0, 0, 0u};
    bool in_kernel_exchange = false;
    // the resident kernel (k_nn_cert<.., LATE>): once the certificate policy is on, the remaining iterations run
    // inside ONE launch, the solve included, until the registration is done or the same policy says leave
    bool late_ok;
    CertPolicy policy;
    IterEvents ev;

    static bool can_cert(const wm_ctx *ctx, const wm_icp_params *p, bool brute) {
        return !brute && ctx->tune_nn_balanced && ctx->tune_cert_from >= -1 && ctx->n_tgt_input < (1u << 26) - 8u &&
               !ctx->cost_log.p && p->mode != WM_ICP_PLANE && p->reject == WM_REJECT_NONE;
    }
    IcpLoop(wm_ctx *c, const wm_icp_params *p_, bool brute_, float thr_, wm_comm *comm_, double *blk_)
        : ctx(c), p(p_), brute(brute_), thr(thr_), comm(comm_), blk(blk_),
          max_it(p_->force_iterations > 0 ? p_->force_iterations : p_->max_iter), nb(stat_blocks(c->n_src)),
          kLag(c->tune_lag >= 1 && c->tune_lag <= 16 ? c->tune_lag : 2), plane(p_->mode == WM_ICP_PLANE),
          reject(p_->reject != WM_REJECT_NONE), slab(c->h_state->slab_on != 0),
          use_bins(!brute_ && c->tune_bins != 0 && !c->cost_log.p && !plane && !reject),
          cert_thr(brute_ ? 0.f : c->tune_cert_disp * c->levels[0].d.h),
          late_ok(can_cert(c, p_, brute_) && c->tune_late && !blk_ && !slab && !c->cert_count.p && !c->cert_prof.p),
          policy(can_cert(c, p_, brute_), c->tune_cert_from, cert_thr, c->tune_cert_changed, c->tune_cert_unsettled, kLag,
                 max_it),
          ev(c, p_->profile, max_it) {}

    // the pinned records of this loop's iterations, all "not written yet"; the bins; the counters of the last align
    int begin() {
        ctx->iter_nn_ms.clear();
        WM_HIP(ctx, hipEventRecord(ctx->ev_a, ctx->stream));
        if (ctx->h_pub_slots < max_it + 1) {
            if (ctx->h_pub) (void) hipHostFree(ctx->h_pub);
            ctx->h_pub = nullptr;
            ctx->h_pub_slots = 0;
            WM_HIP(ctx, hipHostMalloc((void **) &ctx->h_pub, sizeof(unsigned long long) * (size_t) (max_it + 2),
                                      hipHostMallocDefault));
            ctx->h_pub_slots = max_it + 1;
        }
        // (nothing of an earlier align is in flight: each ends with a fetch of the state)
        memset(ctx->h_pub, 0, sizeof(unsigned long long) * (size_t) (max_it + 1));
        in_kernel_exchange = blk && comm_exchange_args(comm, &xchg) == WM_OK;
        ctx->cert_launches = 0;
        if (reject) WM_TRY(reject_ready(ctx));
        if (use_bins) {
            WM_TRY(bins_ready(ctx));  // (zeroes them if the last loop left them dirty)
            ctx->bins_dirty = true;   // (until this loop has ended normally)
        }
        ctx->late_iters = ctx->late_launches = 0;
        ctx->late_ms = 0.f;
        return WM_OK;
    }

    // the record of iteration it - kLag (host_wait's three stages); *have = false: the device is done and stopped
    // before it wrote that one
    int wait_record(int it, StepRecord *rec, bool *have) {
        const unsigned need = (unsigned) (it - kLag + 1);  // iterations finished by then
        volatile unsigned long long *pub = ctx->h_pub;
        unsigned long long w = 0ull;
        const HostWait hw = host_wait(
            ctx,
            [&] {
                w = pub[need];
                if (record_is_for(w, need)) return true;
                // done -- and the record waited for is not one the device wrote before it stopped: nothing more
                // will come.  (The last record and the done word are two relaxed stores of one kernel: seeing
                // `done` first must not end the loop one iteration early -- in the sharded loop every enqueued
                // iteration carries a collective, and all ranks have to issue the same number of them: exactly
                // iterations-finished + kLag.)
                const unsigned long long p0 = pub[0];
                return done_word_done(p0) && need > done_word_iterations(p0);
            },
            std::chrono::milliseconds(20));
        if (hw == kWaitFailed) return WM_ERR_HIP;
        // a long wait (huge clouds, a shared device): the runtime blocked until everything enqueued had run -- the
        // record is there then, unless a kernel failed
        if (hw == kWaitBlocked) w = pub[need];
        *have = record_is_for(w, need);
        if (*have) *rec = unpack_step_record(w);
        return WM_OK;
    }

    // the resident kernel from iteration `it` on: admitted -> launched -> waited for -> released.  *ran < 0: not
    // admitted (the caller launches this iteration); else the iterations it ran, and *go_on whether more follow
    int drive_resident(int it, unsigned late_blocks, int *ran, bool *go_on) {
        *ran = -1;
        const int share = resident_admit(ctx->device, (int) late_blocks, ctx->late_capacity);
        if (share <= 0) return WM_OK;
        hipEvent_t l0 = nullptr, l1 = nullptr;
        if (p->profile) {
            l0 = get_event(ctx, ev.used++);
            l1 = get_event(ctx, ev.used++);
            WM_HIP(ctx, hipEventRecord(l0, ctx->stream));
        }
        const unsigned seq = ++ctx->late_seq;
        // (a forced choice -- tune_cert_from >= 0 -- stays inside whatever the searched share)
        const bool forced_choice = ctx->tune_cert_from >= 0;
        int rc = launch_nn_late(ctx, thr, p->mode, late_blocks, policy.bounds_valid, seq,
                                forced_choice ? 2.f : ctx->tune_cert_unsettled, forced_choice ? 3.0e38f : 3.f * cert_thr,
                                max_it - it);
        if (rc == WM_OK && l1) rc = hipEventRecord(l1, ctx->stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
        if (rc == WM_OK) {  // the host has nothing to decide until it leaves: wait for its word
            volatile unsigned long long *hx = ctx->h_late;
            if (host_wait(ctx, [&] { return (unsigned) (*hx >> 32) == seq; }, std::chrono::milliseconds(20)) == kWaitFailed)
                rc = WM_ERR_HIP;
        }
        resident_release(ctx->device, share);
        if (rc != WM_OK) {
            if (rc == WM_ERR_HIP) ctx->last_error = "resident ICP kernel: launch or wait failed";
            return rc;
        }
        const unsigned long long w = *ctx->h_late;
        if ((unsigned) (w >> 32) != seq) {
            ctx->last_error = "resident ICP kernel: finished without its exit word";
            return WM_ERR_STATE;
        }
        const int reason = (int) ((w >> 24) & 0xFFu), inside = (int) (w & 0xFFFFFFu);
        if (ctx->late_debug_iter >= 0) late_debug_report(ctx, late_blocks, inside, reason);  // developer (WM_LATE_DEBUG)
        if (l0) ev.late.emplace_back(l0, l1);
        ctx->late_launches++;
        ctx->late_iters += inside;
        ctx->cert_launches += inside;
        if (reason == 3) late_ok = false;  // (a wait gave up: launched iterations from here on)
        *go_on = policy.ran_resident(it, inside, reason);  // (false: done -- also: it was queued behind a `done` and ran nothing)
        if (*go_on && inside <= 0 && reason != 3) {  // (cannot happen: it left without a reason to)
            ctx->last_error = "resident ICP kernel: left without running an iteration";
            return WM_ERR_STATE;
        }
        *ran = inside;
        return WM_OK;
    }

    // iteration `it`'s correspondences and its sums: *rows rows of partials, the bins, or (plane) the plane bins
    int enqueue_search(int it, bool cert_on, unsigned *rows) {
        *rows = (unsigned) nb;
        if (reject) {
            if (blk) return WM_ERR_ARG;  // (not sharded: the entry points refuse it)
            if (brute) WM_TRY(launch_nn_brute(ctx, thr, ev.e0, ev.e1));
            else WM_TRY(launch_nn_grid(ctx, thr, ev.e0, ev.e1, ev.e1b, -1, nullptr, false));
            if (brute) WM_TRY(ev.record(ev.e1b));
            WM_TRY(launch_reject_select(ctx, ctx->keys.as<unsigned long long>(), (unsigned) ctx->n_src, p->reject, p->reject_ratio,
                                        p->reject_factor, (unsigned) p->reject_min_corr, 0u));
            return plane ? launch_plane_stats(ctx, reject_threshold(ctx)) : launch_stats(ctx, p->mode, reject_threshold(ctx));
        }
        if (plane) {
            if (blk) return WM_ERR_ARG;  // (not sharded: the entry points refuse the mode)
            if (brute) WM_TRY(launch_nn_brute(ctx, thr, ev.e0, ev.e1));
            else WM_TRY(launch_nn_grid(ctx, thr, ev.e0, ev.e1, ev.e1b, -1, nullptr, false));
            if (brute) WM_TRY(ev.record(ev.e1b));
            return launch_plane_stats(ctx);
        }
        if (brute) {
            WM_TRY(launch_nn_brute(ctx, thr, ev.e0, ev.e1));
            WM_TRY(ev.record(ev.e1b));
            return launch_stats(ctx, p->mode);
        }
        if (!cert_on) {
            WM_TRY(launch_nn_grid(ctx, thr, ev.e0, ev.e1, ev.e1b, p->mode, rows, use_bins));
            (void) policy.ran_full(it);
            return WM_OK;
        }
        if (slab && !policy.bounds_valid) {
            // a rank only ever writes the bounds of the queries it owns at the time: nothing stale
            // may survive a stretch of full searches (or the start)
            WM_HIP(ctx, ctx->nn_bound.reserve(((size_t) ctx->n_src + 64) * sizeof(float4)));
            WM_HIP(ctx, hipMemsetAsync(ctx->nn_bound.p, 0, ((size_t) ctx->n_src + 64) * sizeof(float4), ctx->stream));
        }
        WM_TRY(launch_nn_cert(ctx, thr, ev.e0, ev.e1, ev.e1b, p->mode, rows, policy.bounds_valid || slab, use_bins));
        (void) policy.ran_cert(it);
        ctx->cert_launches++;
        ev.note_cert(it);
        return WM_OK;
    }

    // the sums -> the step, PCL's stopping rules, the iteration's record
    int enqueue_solve(unsigned rows) {
        long long *bins = use_bins ? ctx->bins.as<long long>() : nullptr;
        if (plane) return launch_plane_solve(ctx, ctx->h_pub, ctx->h_pub_slots, 1);
        // sharded, mailboxes: this rank's sums, their exchange with the other ranks over xGMI and the same
        // solve on every rank in ONE launch
        if (blk && in_kernel_exchange) return launch_reduce_solve<7>(ctx, rows, blk, ctx->h_pub, ctx->h_pub_slots, 1, &xchg, bins);
        if (blk) {
            // sharded: this rank's sums -> all-reduce of the block over the ranks (RCCL on this stream) ->
            // the same solve on every rank
            WM_TRY(launch_reduce_solve<1>(ctx, rows, blk, nullptr, 0, 1, nullptr, bins));
            hipEvent_t ea = nullptr, eb = nullptr;
            if (p->profile) {
                ea = get_event(ctx, ev.ar++);
                eb = get_event(ctx, ev.ar++);
            }
            WM_TRY(ev.record(ea));
            WM_TRY(comm_allreduce(ctx, comm, blk, kBlkLen));
            WM_TRY(ev.record(eb));
            return launch_reduce_solve<2>(ctx, 0, blk, ctx->h_pub, ctx->h_pub_slots, 1);
        }
        if (use_bins) return launch_bins_solve(ctx, ctx->h_pub, ctx->h_pub_slots);
        return launch_reduce_solve<3>(ctx, rows, nullptr, ctx->h_pub, ctx->h_pub_slots);
    }

    // behind the last iteration: the ranks' verdict on the exchange, the keys brought up to date, the state
    // fetched; then what the context and the caller keep of it
    int finish(double T_out[16], wm_icp_stats *stats) {
        if (in_kernel_exchange) {  // every rank, whatever it saw: the ranks agree on how the exchange went (k_xchg_commit)
            hipLaunchKernelGGL(k_xchg_commit, dim3(1), dim3(kBlock), 0, ctx->stream, ctx->d_state.as<IcpDevState>(), xchg);
            WM_HIP(ctx, hipGetLastError());
        }
        if (ctx->cert_launches > 0) WM_TRY(launch_fix_keys(ctx, thr));
        // the keys become the kept pairs only now: while the loop ran, an iteration's keys seeded the next search
        if (reject) WM_TRY(launch_reject_mark(ctx));
        WM_TRY(download_state(ctx));
        WM_HIP(ctx, hipEventRecord(ctx->ev_b, ctx->stream));
        WM_HIP(ctx, hipEventSynchronize(ctx->ev_b));
        const IcpDevState &s = *ctx->h_state;
        if (s.xchg_failed) {
            ctx->xchg_timed_out = true;
            ctx->last_error = "sharded registration: a rank's block did not arrive in a mailbox in time, on this rank or -- as "
                              "the commit round told -- on a peer (a rank failed or fell behind by more than the exchange's "
                              "time limit); every rank of the group fails this registration alike";
            return WM_ERR_RCCL;
        }
        if (use_bins) ctx->bins_dirty = false;
        ctx->prev_mse = s.prev_mse;
        ctx->have_corr = true;
        ctx->last_align_valid = true;
        ctx->last_align_converged = s.converged != 0;
        ctx->last_align_sharded = blk != nullptr;
        memcpy(ctx->corr_T, s.T, sizeof(s.T));
        if (stats) {
            stats_from_state(s, stats);
            stats->nn_levels = brute ? 0 : ctx->n_levels;
            stats->grid_cell = brute ? 0.f : ctx->levels[0].d.h;
            stats->deferred = s.deferred_total;
            stats->cert_launches = ctx->cert_launches;
            stats->late_iterations = ctx->late_iters;
            stats->late_launches = ctx->late_launches;
            stats->exchange_in_kernel = in_kernel_exchange ? 1 : 0;
            if (reject) {
                stats->n_matched = s.n_matched;
                memcpy(&stats->reject_d2, &s.reject_bits, sizeof(float));
            }
            (void) hipEventElapsedTime(&stats->align_ms, ctx->ev_a, ctx->ev_b);
            ev.read_back(s, blk != nullptr, stats);
        }
        if (s.state == WM_CONV_NO_CORRESPONDENCES) return WM_TOO_FEW_CORRESPONDENCES;
        if (!s.converged) return WM_NOT_CONVERGED;
        memcpy(T_out, s.T, sizeof(s.T));
        return WM_OK;
    }
};

}  // namespace

// The iteration loop of one registration, from an uploaded state to the fetched result: shared by
// wm_icp_align (blk == nullptr) and the sharded registration (wm_shard.hip: blk = the WM_STATS_LEN
// doubles in HBM that are all-reduced over `comm` between a rank's sums and the solve).
int icp_run_loop(wm_ctx *ctx, const wm_icp_params *p, bool brute, float thr, wm_comm *comm, double *blk,
                 double T_out[16], wm_icp_stats *stats) {
    IcpLoop L(ctx, p, brute, thr, comm, blk);
    WM_TRY(L.begin());
    // The host runs AHEAD of the device, never more than kLag iterations (2: one iteration in flight, one
    // queued behind it -- 4 decided two iterations later when to certify, 3.72 vs 3.69 ms; 1 drains the
    // queue between iterations, 4.04 ms): every solve kernel publishes
    // (done, iterations finished, the size of its step) in one word of pinned memory, and before
    // enqueueing iteration `it` the host waits until iteration it - kLag has been published.  The
    // device always has work queued (no pipeline drain, round 2: one every 8 iterations), iterations
    // enqueued behind a `done` are no-ops, and the host picks the search kernel of iteration `it` from
    // the step size iteration it - kLag recorded (its own record, so the choice does not depend on
    // timing and a registration stays bit-reproducible): the full search (k_nn_grid) while the clouds
    // still move, the certificate kernel (k_nn_cert) once a step is a small fraction of a grid cell.
    // The choice changes the work, never the correspondences.
    for (int it = 0; it < L.max_it; ++it) {
        StepRecord seen;  // what iteration it - kLag recorded (its own record)
        bool have = false;
        if (it >= L.kLag) {
            WM_TRY(L.wait_record(it, &seen, &have));
            if (!have) break;  // done, and that record will not come
        }
        const bool cert_on = L.policy.decide(it, have ? &seen : nullptr);
        unsigned late_blocks = 0;
        if (cert_on && L.late_ok && late_possible(ctx, p->mode, &late_blocks)) {
            int ran = -1;
            bool go_on = true;
            WM_TRY(L.drive_resident(it, late_blocks, &ran, &go_on));
            if (!go_on) break;
            if (ran >= 0) {
                it += ran - 1;  // (the loop's own ++it: on to the first iteration it did not run)
                continue;
            }
        }
        unsigned rows = 0;
        L.ev.begin_iteration(it);
        WM_TRY(L.enqueue_search(it, cert_on, &rows));
        WM_TRY(L.ev.record(L.ev.e2));
        WM_TRY(L.enqueue_solve(rows));
        WM_TRY(L.ev.record(L.ev.e3));
        WM_HIP(ctx, hipGetLastError());
    }
    return L.finish(T_out, stats);
}

// expect < 0: the cloud's count of finite source points arrives in the all-reduced block (the sum of
// the ranks' stripe_finite); see IcpDevState::expect_owned
int shard_begin(wm_ctx *ctx, const wm_icp_params *p, double x_lo, double x_hi, double expect, double stripe_finite,
                bool *brute_out, float *thr_out, double prev_mse0) {
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(finalize_clouds(ctx, p->max_corr, p->nn_method));
    WM_TRY(prepare_work(ctx));
    ctx->shard_brute = use_brute(ctx, p->nn_method) || ctx->n_tgt == 0;
    if (!ctx->shard_brute) WM_TRY(ensure_levels(ctx, p->max_corr));
    ctx->shard_thr = threshold_d2(p->max_corr);
    ctx->shard_params = *p;
    double I[16];
    mat4_identity(I);
    init_state(ctx->h_state, I, p, prev_mse0);
    ctx->h_state->svd_warm = 1;
    ctx->h_state->slab_on = 1;
    ctx->h_state->slab_lo = x_lo < -3.0e38 ? -INFINITY : (float) x_lo;
    ctx->h_state->slab_hi = x_hi > 3.0e38 ? INFINITY : (float) x_hi;
    ctx->h_state->expect_owned = expect;
    ctx->h_state->stripe_finite = stripe_finite;
    set_step_scale(ctx);
    // keys / matches double as next iteration's candidates: start from "nothing known" (a rank only ever
    // writes the entries of the queries it owns at the time)
    const size_t n1 = ctx->n_src > 0 ? ctx->n_src : 1;
    WM_HIP(ctx, hipMemsetAsync(ctx->keys.p, 0xFF, n1 * sizeof(unsigned long long), ctx->stream));
    WM_HIP(ctx, hipMemsetAsync(ctx->match_pt.p, 0xFF, n1 * sizeof(float4), ctx->stream));
    WM_TRY(upload_state(ctx));
    ctx->iter_nn_ms.clear();
    ctx->shard_active = true;
    if (brute_out) *brute_out = ctx->shard_brute;
    if (thr_out) *thr_out = ctx->shard_thr;
    return WM_OK;
}

}  // namespace wm

using namespace wm;

// =============================================================== C ABI
extern "C" {

void wm_icp_default_params(wm_icp_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_corr = 3;    // icp.hpp:35
    p->max_iter = 100;  // icp.hpp:37
    p->t_eps = 1e-8;    // icp.hpp:41
    p->fit_eps = 1e-2;  // icp.hpp:43
    p->mode = WM_ICP_SVD;
    p->nn_method = WM_NN_AUTO;
    p->carry_state = 1;
    p->reject = WM_REJECT_NONE;
    p->reject_ratio = 0.5;   // CorrespondenceRejectorTrimmed's overlap_ratio_
    p->reject_factor = 1.0;  // CorrespondenceRejectorMedianDistance's factor_
    p->reject_min_corr = 0;
}

int wm_icp_align(wm_ctx *ctx, const wm_icp_params *p, double T_out[16], wm_icp_stats *stats) {
    if (!ctx || !p || !T_out) return WM_ERR_ARG;
    if (!(p->max_corr > 0) || (p->mode != WM_ICP_SVD && p->mode != WM_ICP_GN6 && p->mode != WM_ICP_PLANE)) return WM_ERR_ARG;
    if (p->force_iterations <= 0 && p->max_iter <= 0) return WM_ERR_ARG;
    if (p->mode == WM_ICP_PLANE && (plane_normal_k(p->normal_k) < 3 || plane_normal_k(p->normal_k) > 32)) return WM_ERR_ARG;
    if (!reject_params_ok(p->reject, p->reject_ratio, p->reject_factor, p->reject_min_corr)) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (ctx->n_src_input == 0 || ctx->n_tgt_input == 0) {
        // PCL: empty input -> "Not enough correspondences"; match() returns false
        if (stats) stats->state = WM_CONV_NO_CORRESPONDENCES;
        return ctx->n_tgt_input == 0 && ctx->n_src_input == 0 ? WM_ERR_STATE
                                                               : WM_TOO_FEW_CORRESPONDENCES;
    }
    WM_TRY(finalize_clouds(ctx, p->max_corr, p->nn_method));
    if (ctx->n_src == 0 || ctx->n_tgt == 0) {
        if (stats) stats->state = WM_CONV_NO_CORRESPONDENCES;
        return WM_TOO_FEW_CORRESPONDENCES;
    }
    WM_TRY(prepare_work(ctx));
    const bool brute = use_brute(ctx, p->nn_method);
    if (!brute) WM_TRY(ensure_levels(ctx, p->max_corr));
    if (p->mode == WM_ICP_PLANE) {
        // the target's normals, once per target (and k): cached on the context until wm_set_target
        const int rc = plane_target_normals(ctx, p->normal_k);
        if (rc == WM_NOT_CONVERGED && stats) stats->state = WM_CONV_NO_CORRESPONDENCES;  // fewer target points than neighbours
        if (rc != WM_OK) return rc == WM_NOT_CONVERGED ? WM_TOO_FEW_CORRESPONDENCES : rc;
        WM_TRY(plane_bins_ready(ctx));
    }
    const float thr = threshold_d2(p->max_corr);
    double I[16];
    mat4_identity(I);
    const double prev = (p->carry_state && ctx->prev_mse >= 0) ? ctx->prev_mse : DBL_MAX;
    init_state(ctx->h_state, I, p, prev);
    ctx->h_state->svd_warm = 1;
    set_step_scale(ctx);
    WM_TRY(upload_state(ctx));

    return icp_run_loop(ctx, p, brute, thr, nullptr, nullptr, T_out, stats);
}

static int unpack_correspondences(wm_ctx *ctx, int32_t *match_idx, float *d2, size_t cap) {
    const size_t n_in = ctx->n_src_input;
    if (cap < n_in) return WM_ERR_ARG;
    if (n_in == 0) return WM_OK;
    WM_HIP(ctx, ctx->corr_tmp_idx.reserve(n_in * sizeof(int)));
    WM_HIP(ctx, ctx->corr_tmp_d2.reserve(n_in * sizeof(float)));
    // dropped (non-finite) source points keep "no match"
    WM_HIP(ctx, hipMemsetAsync(ctx->corr_tmp_idx.p, 0xFF, n_in * sizeof(int), ctx->stream));
    WM_HIP(ctx, hipMemsetAsync(ctx->corr_tmp_d2.p, 0, n_in * sizeof(float), ctx->stream));
    const unsigned n = (unsigned) ctx->n_src;
    if (n > 0) {
        hipLaunchKernelGGL(k_unpack_corr, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0,
                           ctx->stream, ctx->src_sorted.as<float4>(), n,
                           ctx->keys.as<unsigned long long>(), ctx->corr_tmp_idx.as<int>(),
                           ctx->corr_tmp_d2.as<float>());
        WM_HIP(ctx, hipGetLastError());
    }
    if (match_idx) WM_TRY(copy_to_caller(ctx, match_idx, ctx->corr_tmp_idx.p, n_in * sizeof(int)));
    if (d2) WM_TRY(copy_to_caller(ctx, d2, ctx->corr_tmp_d2.p, n_in * sizeof(float)));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

int wm_icp_match(wm_ctx *ctx, const void *ref, size_t n_ref, const void *target, size_t n_target,
                 size_t stride, int mem, const wm_icp_params *p, float res, int multiscale_steps,
                 double T_out[16], wm_icp_stats *stats) {
    if (!ctx || !p || !T_out || (n_ref > 0 && !ref) || (n_target > 0 && !target) || stride < 12 ||
        (stride & 3) || n_ref > 0x7FFFFFF0u || n_target > 0x7FFFFFF0u)
        return WM_ERR_ARG;
    if (!reject_params_ok(p->reject, p->reject_ratio, p->reject_factor, p->reject_min_corr)) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!(res > 0)) {  // icp.cpp:123-131
        WM_TRY(wm_set_source(ctx, ref, n_ref, stride, mem));
        WM_TRY(wm_set_target(ctx, target, n_target, stride, mem));
        return wm_icp_align(ctx, p, T_out, stats);
    }
    const size_t cap_r = n_ref > 0 ? n_ref : 1, cap_t = n_target > 0 ? n_target : 1;
    WM_HIP(ctx, ctx->match_ref.reserve(cap_r * sizeof(float4)));
    WM_HIP(ctx, ctx->match_tgt.reserve(cap_t * sizeof(float4)));
    WM_HIP(ctx, ctx->ds_ref.reserve(cap_r * sizeof(float4)));
    WM_HIP(ctx, ctx->ds_tgt.reserve(cap_t * sizeof(float4)));
    float4 *d_ref = ctx->match_ref.as<float4>(), *d_tgt = ctx->match_tgt.as<float4>();
    float4 *ds_ref = ctx->ds_ref.as<float4>(), *ds_tgt = ctx->ds_tgt.as<float4>();
    WM_TRACE(ctx, "match: begin");
    WM_TRY(pack_cloud(ctx, ref, n_ref, stride, mem, d_ref));
    WM_TRACE(ctx, "match: packed ref");
    WM_TRY(pack_cloud(ctx, target, n_target, stride, mem, d_tgt));
    WM_TRACE(ctx, "match: packed target");
    wm_icp_params prm = *p;
    wm_icp_stats last, total;
    memset(&total, 0, sizeof(total));
    double running[16];
    mat4_identity(running);
    const int steps = multiscale_steps > 0 ? multiscale_steps : 0;
    // both clouds are filtered once per scale: their bounding boxes are found once
    VgKnown kr{}, kt{};
    if (steps > 0) {
        if (n_ref > 0) WM_TRY(compute_bbox(ctx, d_ref, n_ref, &kr.bb, &kr.valid));
        if (n_target > 0) WM_TRY(compute_bbox(ctx, d_tgt, n_target, &kt.bb, &kt.valid));
    }
    for (int i = steps; i >= 0; --i) {
        const float leaf = (float) (pow(2, i) * res);  // icp.cpp:80
        size_t nr = 0, nt = 0;
        WM_TRY(voxel_downsample_dev(ctx, d_ref, n_ref, leaf, ds_ref, &nr, steps > 0 && n_ref > 0 ? &kr : nullptr));
        WM_TRACE(ctx, "match: voxel ref");
        WM_TRY(voxel_downsample_dev(ctx, d_tgt, n_target, leaf, ds_tgt, &nt, steps > 0 && n_target > 0 ? &kt : nullptr));
        WM_TRACE(ctx, "match: voxel target");
        if (ctx->trace) fprintf(stderr, "[wm] match: leaf=%g nr=%zu nt=%zu\n", leaf, nr, nt);
        if (steps > 0) {
            WM_TRY(transform_cloud_dev(ctx, ds_ref, nr, running, ds_ref));  // icp.cpp:84-86
            WM_TRACE(ctx, "match: transformed");
            prm.max_corr = pow(2, i) * p->max_corr;                          // icp.cpp:93-94
        }
        WM_TRY(wm_set_source(ctx, ds_ref, nr, sizeof(float4), WM_MEM_DEVICE));
        WM_TRACE(ctx, "match: set_source");
        WM_TRY(wm_set_target(ctx, ds_tgt, nt, sizeof(float4), WM_MEM_DEVICE));
        WM_TRACE(ctx, "match: set_target");
        double Ti[16];
        const int rc = wm_icp_align(ctx, &prm, Ti, &last);
        WM_TRACE(ctx, "match: align");
        total.align_ms += last.align_ms;
        total.nn_ms += last.nn_ms;
        total.nn_launches += last.nn_launches;
        if (stats) {
            const float a = total.align_ms, b = total.nn_ms;
            const int c = total.nn_launches;
            *stats = last;
            stats->align_ms = a;
            stats->nn_ms = b;
            stats->nn_launches = c;
        }
        if (rc != WM_OK) return rc;  // icp.cpp:96-98: fail fast, result untouched
        mat4_mul(Ti, running, running);  // icp.cpp:99-101
    }
    memcpy(T_out, running, sizeof(running));
    return WM_OK;
}

// ------------------------------------------------ sharded (multi-GPU) stepping
int wm_icp_shard_begin(wm_ctx *ctx, const wm_icp_params *p, double x_lo, double x_hi,
                       size_t expect_owned_total) {
    // (an empty slab, x_lo == x_hi, and an empty band of the source are legitimate for a rank of a
    // sharded registration: it contributes zeros)
    if (!ctx || !p || !(p->max_corr > 0) || !(x_lo <= x_hi)) return WM_ERR_ARG;
    if (p->mode == WM_ICP_PLANE) return WM_ERR_ARG;  // (the plane metric is not sharded)
    if (p->reject != WM_REJECT_NONE) return WM_ERR_ARG;  // (nor is correspondence rejection)
    if (ctx->n_src_input == 0 && expect_owned_total == 0) return WM_ERR_STATE;
    WM_TRY(shard_begin(ctx, p, x_lo, x_hi, (double) expect_owned_total, 0.0, nullptr, nullptr, DBL_MAX));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

int wm_icp_shard_local_stats(wm_ctx *ctx, void *stats_dev) {
    if (!ctx || !stats_dev) return WM_ERR_ARG;
    if (!ctx->shard_active) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->shard_params.profile) {
        const size_t k = ctx->iter_nn_ms.size();
        e0 = get_event(ctx, 2 * k);
        e1 = get_event(ctx, 2 * k + 1);
        ctx->iter_nn_ms.push_back(-1.f);
    }
    unsigned rows = 0;
    if (ctx->n_src > 0) {
        if (ctx->shard_brute) {
            WM_TRY(launch_nn_brute(ctx, ctx->shard_thr, e0, e1));
            WM_TRY(launch_stats(ctx, ctx->shard_params.mode));
            rows = (unsigned) stat_blocks(ctx->n_src);
        } else {
            WM_TRY(launch_nn_grid(ctx, ctx->shard_thr, e0, e1, nullptr, ctx->shard_params.mode, &rows));
        }
    }
    return launch_reduce_solve<1>(ctx, rows, static_cast<double *>(stats_dev));
}

int wm_icp_shard_apply(wm_ctx *ctx, const void *stats_dev) {
    if (!ctx || !stats_dev) return WM_ERR_ARG;
    if (!ctx->shard_active) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    return launch_reduce_solve<2>(ctx, 0, const_cast<double *>(static_cast<const double *>(stats_dev)));
}

int wm_icp_shard_poll(wm_ctx *ctx, int *done, double T_out[16], wm_icp_stats *stats) {
    if (!ctx) return WM_ERR_ARG;
    if (!ctx->shard_active) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(download_state(ctx));
    const IcpDevState &s = *ctx->h_state;
    if (done) *done = s.done;
    if (T_out) memcpy(T_out, s.T, sizeof(s.T));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats_from_state(s, stats);
        stats->deferred = s.deferred_total;
        stats->nn_levels = ctx->shard_brute ? 0 : ctx->n_levels;
        stats->grid_cell = ctx->shard_brute ? 0.f : ctx->levels[0].d.h;
        if (ctx->shard_params.profile) {
            for (size_t k = 0; k < ctx->iter_nn_ms.size(); ++k) {
                float ms = 0;
                if (ctx->n_src > 0 &&
                    hipEventElapsedTime(&ms, ctx->ev_pool[2 * k], ctx->ev_pool[2 * k + 1]) == hipSuccess) {
                    ctx->iter_nn_ms[k] = ms;
                    stats->nn_ms += ms;
                    stats->nn_launches += 1;
                }
            }
        }
    }
    if (s.done) {
        ctx->have_corr = true;
        ctx->last_align_valid = true;
        ctx->last_align_converged = s.converged != 0;
        memcpy(ctx->corr_T, s.T, sizeof(s.T));
    }
    if (s.state == WM_CONV_NO_CORRESPONDENCES) return WM_TOO_FEW_CORRESPONDENCES;
    if (s.done && !s.converged) return WM_NOT_CONVERGED;
    return WM_OK;
}

// ------------------------------------------------ host-only ICP state machine
struct wm_host_icp {
    IcpDevState st;
};

int wm_host_icp_create(wm_host_icp **out, const wm_icp_params *p, size_t expect_owned_total) {
    if (!out || !p) return WM_ERR_ARG;
    wm_host_icp *h = new (std::nothrow) wm_host_icp();
    if (!h) return WM_ERR_NOMEM;
    double I[16];
    mat4_identity(I);
    init_state(&h->st, I, p, DBL_MAX);
    h->st.svd_warm = 1;
    h->st.expect_owned = (double) expect_owned_total;
    *out = h;
    return WM_OK;
}

void wm_host_icp_destroy(wm_host_icp *h) { delete h; }

int wm_host_icp_apply(wm_host_icp *h, const double stats[WM_STATS_LEN]) {
    if (!h || !stats) return WM_ERR_ARG;
    if (h->st.done) return WM_OK;
    icp_apply_stats(&h->st, stats);
    return WM_OK;
}

int wm_host_icp_get(const wm_host_icp *h, int *done, double T_out[16], wm_icp_stats *stats) {
    if (!h) return WM_ERR_ARG;
    if (done) *done = h->st.done;
    if (T_out) memcpy(T_out, h->st.T, sizeof(h->st.T));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats_from_state(h->st, stats);
    }
    return WM_OK;
}

int wm_get_correspondences(wm_ctx *ctx, int32_t *match_idx, float *d2, size_t cap) {
    if (!ctx) return WM_ERR_ARG;
    if (!ctx->have_corr) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    return unpack_correspondences(ctx, match_idx, d2, cap);
}

int wm_nn_search(wm_ctx *ctx, const double T[16], double max_corr, int nn_method,
                 int32_t *match_idx, float *d2, size_t cap, float *kernel_ms) {
    if (!ctx || !T || !(max_corr > 0)) return WM_ERR_ARG;
    if (ctx->n_src_input == 0 || ctx->n_tgt_input == 0) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(finalize_clouds(ctx, max_corr, nn_method & ~WM_NN_WARM));
    WM_TRY(prepare_work(ctx));
    const bool warm = (nn_method & WM_NN_WARM) && ctx->have_corr;
    nn_method &= ~WM_NN_WARM;
    const bool brute = use_brute(ctx, nn_method) || ctx->n_tgt == 0;
    if (!brute) WM_TRY(ensure_levels(ctx, max_corr));
    init_state(ctx->h_state, T, nullptr, DBL_MAX);
    ctx->h_state->have_prev = warm ? 1 : 0;
    WM_TRY(upload_state(ctx));
    const float thr = threshold_d2(max_corr);
    hipEvent_t e0 = kernel_ms ? ctx->ev_a : nullptr, e1 = kernel_ms ? ctx->ev_b : nullptr;
    if (brute)
        WM_TRY(launch_nn_brute(ctx, thr, e0, e1));
    else
        WM_TRY(launch_nn_grid(ctx, thr, e0, e1, nullptr));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (kernel_ms) (void) hipEventElapsedTime(kernel_ms, ctx->ev_a, ctx->ev_b);
    ctx->have_corr = true;
    ctx->last_align_valid = false;
    memcpy(ctx->corr_T, T, sizeof(double) * 16);
    if (match_idx || d2) return unpack_correspondences(ctx, match_idx, d2, cap);
    return WM_OK;
}

int wm_icp_stats_for(wm_ctx *ctx, const double T[16], int mode, double stats[WM_STATS_LEN]) {
    if (!ctx || !T || !stats || (mode != WM_ICP_SVD && mode != WM_ICP_GN6 && mode != WM_ICP_PLANE)) return WM_ERR_ARG;
    if (!ctx->have_corr) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(prepare_work(ctx));
    wm_icp_params p;
    wm_icp_default_params(&p);
    p.mode = mode;
    init_state(ctx->h_state, T, &p, DBL_MAX);
    WM_TRY(upload_state(ctx));
    if (mode == WM_ICP_PLANE) {
        // the normals the context holds (those of the last plane align or wm_estimate_normals); none yet: the default k
        WM_TRY(plane_target_normals(ctx, ctx->plane_nrm_valid ? ctx->plane_nrm_k : 0));
        WM_TRY(plane_bins_ready(ctx));
        WM_TRY(launch_plane_stats(ctx));
        WM_TRY(launch_plane_solve(ctx, nullptr, 0, 0));
        WM_TRY(download_state(ctx));
        memcpy(stats, ctx->h_state->stats, sizeof(double) * WM_STATS_LEN);
        return WM_OK;
    }
    WM_TRY(launch_stats(ctx, mode));
    WM_TRY(launch_reduce_solve<1>(ctx, (unsigned) stat_blocks(ctx->n_src), nullptr));
    WM_TRY(download_state(ctx));
    memcpy(stats, ctx->h_state->stats, sizeof(double) * WM_STATS_LEN);
    return WM_OK;
}

int wm_umeyama_from_stats(const double stats[WM_STATS_LEN], double Tk_out[16]) {
    if (!stats || !Tk_out) return WM_ERR_ARG;
    if (!(stats[0] >= 3.0)) return WM_TOO_FEW_CORRESPONDENCES;
    umeyama_from_stats(stats, Tk_out);
    return WM_OK;
}

int wm_gn6_from_stats(const double stats[WM_STATS_LEN], double Tk_out[16]) {
    if (!stats || !Tk_out) return WM_ERR_ARG;
    if (!(stats[0] >= 3.0)) return WM_TOO_FEW_CORRESPONDENCES;
    return gn6_from_stats(stats, Tk_out) ? WM_OK : WM_NOT_CONVERGED;
}

}  // extern "C"
