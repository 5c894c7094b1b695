// wm_debug.hip -- developer output and introspection: the wm_debug_* logs a test or a profile script arms and reads,
// the per-iteration times of a profiled align, and the resident ICP kernel's stamp report (WM_LATE_DEBUG).
#include "wm_internal.hpp"
#include "wm_bins.hpp"

#include <algorithm>
#include <vector>

#include <math.h>

namespace wm {

// the resident kernel's stamps after a launch of it (icp_run_loop, wm_icp.hip): the solver's of every iteration, the
// workers' of iteration WM_LATE_DEBUG (100 MHz wall clock)
void late_debug_report(wm_ctx *ctx, unsigned late_blocks, int inside, int reason) {
    unsigned long long d[64 * 4];
    (void) hipStreamSynchronize(ctx->stream);
    if (hipMemcpy(d, (char *) ctx->late_ctl.p + late_ctl_bytes(), sizeof(d), hipMemcpyDeviceToHost) == hipSuccess) {
        fprintf(stderr, "[wm] late kernel: %d iterations, reason %d\n", inside, reason);
        for (int k = 0; k < inside && k < 64; ++k)
            fprintf(stderr, "  it %2d: workers (hand-out -> all rows in) %6.2f us | rows added %5.2f | solve %5.2f | hand-out %5.2f\n", k,
                    k ? ((long long) d[k * 4] - (long long) d[(k - 1) * 4 + 3]) * 0.01 : 0.0,
                    (d[k * 4 + 1] - d[k * 4]) * 0.01, (d[k * 4 + 2] - d[k * 4 + 1]) * 0.01,
                    (d[k * 4 + 3] - d[k * 4 + 2]) * 0.01);
        // the workers' stamps of iteration WM_LATE_DEBUG, relative to the solver's hand-out before it
        const int li = ctx->late_debug_iter;
        std::vector<unsigned long long> wst((size_t) late_blocks * 8);
        if (li >= 1 && li < inside && li < 64 && ctx->cert_prof.p &&
            hipMemcpy(wst.data(), ctx->cert_prof.p, wst.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            const unsigned long long t0 = d[(li - 1) * 4 + 3];
            const char *names[6] = {"pose in", "phase 1 done", "wave 0 searched", "all searched + stored", "row stored", "ticket drawn"};
            for (int k = 0; k < 6; ++k) {
                double mx = 0, mn = 1e30;
                std::vector<double> v;
                for (unsigned b = 0; b < late_blocks; ++b) {
                    const double x = ((long long) wst[(size_t) b * 8 + k] - (long long) t0) * 0.01;
                    v.push_back(x);
                    mx = x > mx ? x : mx;
                    mn = x < mn ? x : mn;
                }
                std::sort(v.begin(), v.end());
                fprintf(stderr, "  it %d workers, %-22s: min %6.2f  median %6.2f  p90 %6.2f  p99 %6.2f  max %6.2f us after the hand-out\n", li,
                        names[k], mn, v[v.size() / 2], v[v.size() * 9 / 10], v[v.size() * 99 / 100], mx);
            }
            std::vector<std::pair<double, unsigned>> slow;
            for (unsigned b = 0; b < late_blocks; ++b)
                slow.emplace_back(((long long) wst[(size_t) b * 8 + 3] - (long long) wst[(size_t) b * 8 + 1]) * 0.01, (unsigned) wst[(size_t) b * 8 + 6]);
            std::sort(slow.begin(), slow.end());
            fprintf(stderr, "  searches (phase 1 done -> all stored), slowest five [us, searched]:");
            for (size_t k = slow.size() >= 5 ? slow.size() - 5 : 0; k < slow.size(); ++k) fprintf(stderr, " %.2f/%u", slow[k].first, slow[k].second);
            double su = 0;
            for (auto &x : slow) su += x.second;
            fprintf(stderr, "; median %.2f/%u; searched per workgroup: mean %.1f\n", slow[slow.size() / 2].first, slow[slow.size() / 2].second, su / slow.size());
        }
    }
}

}  // namespace wm

using namespace wm;

extern "C" {

int wm_debug_cost_log(wm_ctx *ctx, int iterations, unsigned *out, size_t cap) {
    if (!ctx || iterations < 0) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!out) {  // arm: the next align records the search cost of its first `iterations` iterations
        WM_TRY(finalize_clouds(ctx));
        if (iterations == 0) {
            WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
            ctx->cost_log.release();
            ctx->phase_log.release();
            ctx->cost_log_cap = 0;
            return WM_OK;
        }
        WM_HIP(ctx, ctx->cost_log.reserve((size_t) iterations * (ctx->n_src > 0 ? ctx->n_src : 1) * 4));
        WM_HIP(ctx, ctx->phase_log.reserve((size_t) iterations * 8 * sizeof(unsigned long long)));
        WM_HIP(ctx, hipMemsetAsync(ctx->phase_log.p, 0, (size_t) iterations * 8 * sizeof(unsigned long long), ctx->stream));
        ctx->cost_log_iter = 0;
        ctx->cost_log_cap = iterations;
        return WM_OK;
    }
    const size_t need = (size_t) ctx->cost_log_iter * ctx->n_src;
    if (cap < need) return WM_ERR_ARG;
    WM_TRY(copy_to_caller(ctx, out, ctx->cost_log.p, need * 4));
    return ctx->cost_log_iter;
}

int wm_debug_phase_log(wm_ctx *ctx, unsigned long long *out, int iterations) {
    if (!ctx || !out || iterations < 0 || !ctx->phase_log.p) return WM_ERR_ARG;
    if (iterations > ctx->cost_log_iter) iterations = ctx->cost_log_iter;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_TRY(copy_to_caller(ctx, out, ctx->phase_log.p, (size_t) iterations * 8 * sizeof(unsigned long long)));
    return iterations;
}

int wm_debug_solve_cycles(wm_ctx *ctx, unsigned long long out[8]) {
    if (!ctx || !out || !ctx->h_state) return WM_ERR_ARG;
    for (int k = 0; k < 8; ++k) out[k] = ctx->h_state->dbg[k];
    return WM_OK;
}

int wm_debug_bins_sum(const double *x, size_t n, const unsigned *perm, double *out, long long limbs_out[3]) {
    if (!out || (n > 0 && !x)) return WM_ERR_ARG;
    std::vector<long long> bins(kBinWords, 0ll);
    for (size_t k = 0; k < n; ++k) {
        const size_t i = perm ? perm[k] : k;
        if (i >= n) return WM_ERR_ARG;
        const double v = x[i];
        if (!(fabs(v) < 4611686018427387904.0)) return WM_ERR_ARG;
        long long l[kBinLimbs];
        bins_split(v, l);
        const size_t bin = k % (size_t) kBinCount;  // (any assignment of addends to bins gives the same totals)
        for (int j = 0; j < kBinLimbs; ++j) bins[(bin * kBinLimbs + (size_t) j) * kBinStride] += l[j];
    }
    long long L[kBinLimbs] = {0, 0, 0};
    for (int b = 0; b < kBinCount; ++b)
        for (int j = 0; j < kBinLimbs; ++j) L[j] += bins[((size_t) b * kBinLimbs + (size_t) j) * kBinStride];
    *out = bins_value(L[0], L[1], L[2]);
    if (limbs_out)
        for (int j = 0; j < kBinLimbs; ++j) limbs_out[j] = L[j];
    return WM_OK;
}

int wm_debug_cert_log(wm_ctx *ctx, int iterations, unsigned *out, int cap) {
    if (!ctx || iterations < 0) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (!out) {  // arm: the next aligns count the queries k_nn_cert had to search, launch by launch
        WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->cert_log_iter = 0;
        ctx->cert_log_cap = 0;
        if (iterations == 0) {
            ctx->cert_count.release();
            return WM_OK;
        }
        WM_HIP(ctx, ctx->cert_count.reserve((size_t) iterations * 64 * sizeof(unsigned)));
        WM_HIP(ctx, hipMemsetAsync(ctx->cert_count.p, 0, (size_t) iterations * 64 * sizeof(unsigned), ctx->stream));
        if (ctx->cert_prof_on) {
            WM_HIP(ctx, ctx->cert_prof.reserve((size_t) iterations * 64 * sizeof(unsigned long long)));
            WM_HIP(ctx, hipMemsetAsync(ctx->cert_prof.p, 0, (size_t) iterations * 64 * sizeof(unsigned long long), ctx->stream));
        }
        ctx->cert_log_cap = iterations;
        return WM_OK;
    }
    const int n = ctx->cert_log_iter < cap ? ctx->cert_log_iter : cap;
    std::vector<unsigned> tmp((size_t) (n > 0 ? n : 1) * 64);
    if (n > 0) WM_TRY(copy_to_caller(ctx, tmp.data(), ctx->cert_count.p, (size_t) n * 64 * sizeof(unsigned)));
    for (int i = 0; i < n; ++i) {
        unsigned t = 0;
        for (int k = 0; k < 64; ++k) t += tmp[(size_t) i * 64 + k];
        out[i] = t;
    }
    return n;
}

int wm_debug_pub_log(wm_ctx *ctx, unsigned long long *out, int cap) {
    if (!ctx || !out || !ctx->h_pub) return WM_ERR_ARG;
    const int n = ctx->h_pub_slots < cap ? ctx->h_pub_slots : cap;
    for (int k = 0; k < n; ++k) out[k] = ctx->h_pub[k];
    return n;
}

int wm_debug_cert_prof(wm_ctx *ctx, unsigned long long *out, int cap) {
    if (!ctx || !out || !ctx->cert_prof.p) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    const int n = ctx->cert_log_iter < cap ? ctx->cert_log_iter : cap;
    if (n > 0) WM_TRY(copy_to_caller(ctx, out, ctx->cert_prof.p, (size_t) n * 64 * sizeof(unsigned long long)));
    return n;
}

int wm_debug_grid_level(wm_ctx *ctx, int level, double max_corr, float geom[5], int dims[3], size_t *n_points,
                        unsigned *cell_start, size_t cell_cap, float *pts, size_t pts_cap) {
    if (!ctx || level < 0 || level >= kMaxLevels || !geom || !dims || !n_points) return WM_ERR_ARG;
    if (ctx->n_tgt_input == 0) return WM_ERR_STATE;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    if (max_corr > 0) {
        WM_TRY(finalize_clouds(ctx));
        WM_TRY(ensure_levels(ctx, max_corr));
    }
    if (level >= ctx->n_levels || !ctx->levels[level].built) return WM_ERR_STATE;
    const GridLevel &l = ctx->levels[level];
    geom[0] = l.d.ox, geom[1] = l.d.oy, geom[2] = l.d.oz, geom[3] = l.d.h, geom[4] = l.d.inv_h;
    dims[0] = l.d.nx, dims[1] = l.d.ny, dims[2] = l.d.nz;
    unsigned total = 0;
    WM_TRY(copy_to_caller(ctx, &total, l.cell_start.as<unsigned>() + l.ncells, sizeof(unsigned)));
    *n_points = total;
    if ((cell_start && cell_cap < l.ncells + 1) || (pts && pts_cap < (size_t) total + 4)) return WM_ERR_ARG;
    if (cell_start) WM_TRY(copy_to_caller(ctx, cell_start, l.cell_start.p, (l.ncells + 1) * sizeof(unsigned)));
    if (pts) WM_TRY(copy_to_caller(ctx, pts, l.pts.p, ((size_t) total + 4) * sizeof(float4)));
    return WM_OK;
}

int wm_get_iteration_times(wm_ctx *ctx, float *nn_ms, int cap) {
    if (!ctx || !nn_ms || cap < 0) return 0;
    int n = (int) ctx->iter_nn_ms.size();
    if (n > cap) n = cap;
    for (int i = 0; i < n; ++i) nn_ms[i] = ctx->iter_nn_ms[i];
    return n;
}

}  // extern "C"
