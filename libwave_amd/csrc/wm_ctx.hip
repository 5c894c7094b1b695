// wm_ctx.hip -- the context: its life (wm_ctx_create / wm_ctx_destroy / wm_ctx_set_stream), its options by name
// (kOptions, wm_set_option), its clouds (wm_set_source / wm_set_target and finalize_clouds, which fetches what they
// left pending and orders the source) and the one-off correspondence pass over them (nn_pass).
#include "wm_internal.hpp"

#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <new>

namespace wm {

int prepare_work(wm_ctx *ctx) {
    const size_t n = ctx->n_src > 0 ? ctx->n_src : 1;
    WM_HIP(ctx, ctx->keys.reserve(n * sizeof(unsigned long long)));
    WM_HIP(ctx, ctx->match_pt.reserve(n * sizeof(float4)));
    // rows of the fused search + statistics kernel: one per workgroup (at most one per 64 queries, plus grid padding)
    WM_HIP(ctx, ctx->partials.reserve((n / 64 + 1024) * kAcc * sizeof(double)));
    WM_HIP(ctx, ctx->d_state.reserve(sizeof(IcpDevState)));
    if (!ctx->h_state)
        WM_HIP(ctx, hipHostMalloc((void **) &ctx->h_state, sizeof(IcpDevState), hipHostMallocDefault));
    return WM_OK;
}

bool use_brute(const wm_ctx *ctx, int nn_method) {
    if (nn_method == WM_NN_BRUTE) return true;
    if (nn_method == WM_NN_GRID) return false;
    // all-pairs is cheaper than indexing below ~4M pair tests
    return (double) ctx->n_src * (double) ctx->n_tgt_input <= 4.0e6;
}

hipEvent_t get_event(wm_ctx *ctx, size_t k) {
    while (ctx->ev_pool.size() <= k) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ctx->ev_pool.push_back(e);
    }
    return ctx->ev_pool[k];
}

int nn_pass(wm_ctx *ctx, const double T[16], float thr_d2, double max_corr, bool predict, bool slab, float slab_lo,
            float slab_hi, bool wait) {
    WM_TRY(finalize_clouds(ctx, max_corr, WM_NN_AUTO));
    WM_TRY(prepare_work(ctx));
    const bool brute = use_brute(ctx, WM_NN_AUTO) || ctx->n_tgt == 0;
    if (!brute) WM_TRY(ensure_levels(ctx, max_corr));
    float keep_search[12];
    for (int k = 0; k < 12; ++k) keep_search[k] = ctx->h_state->Tf_search[k];
    init_state(ctx->h_state, T, nullptr, DBL_MAX);
    for (int k = 0; k < 12; ++k) ctx->h_state->Tf_search[k] = keep_search[k];  // (still what the align's keys refer to)
    ctx->h_state->have_prev = predict ? 1 : 0;
    if (slab) {  // a rank of a sharded registration searches the queries it owns under this pose
        ctx->h_state->slab_on = 1;
        ctx->h_state->slab_lo = slab_lo;
        ctx->h_state->slab_hi = slab_hi;
    }
    WM_TRY(upload_state(ctx));
    if (brute)
        WM_TRY(launch_nn_brute(ctx, thr_d2, nullptr, nullptr));
    else
        WM_TRY(launch_nn_grid(ctx, thr_d2, nullptr, nullptr, nullptr));
    // (wait = false: the caller queues more work behind the search and waits for that)
    if (wait) WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WM_OK;
}

int join_source_sort(wm_ctx *ctx) {
    if (!ctx->sort_join_pending) return WM_OK;
    ctx->sort_join_pending = false;
    WM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    return WM_OK;
}

// the source's Morton sort that finalize_clouds (mode 2) left for later: on the side stream, behind ev_fork
int enqueue_deferred_sort(wm_ctx *ctx) {
    if (!ctx->sort_deferred) return WM_OK;
    ctx->sort_deferred = false;
    hipStream_t main_stream = ctx->stream;
    ctx->stream = ctx->side_stream;
    const int rc = morton_sort(ctx, ctx->src_orig.as<float4>(), ctx->n_src_input, ctx->src_bbox, ctx->n_src,
                               ctx->src_sorted.as<float4>());
    ctx->stream = main_stream;
    if (rc != WM_OK) return rc;
    WM_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->side_stream));
    ctx->sort_join_pending = true;
    return WM_OK;
}

int finalize_clouds(wm_ctx *ctx, double max_corr, int nn_method, int sort_aside) {
    WM_TRY(enqueue_deferred_sort(ctx));  // (left behind by a call that failed before it got there)
    WM_TRY(join_source_sort(ctx));  // (left behind by a call that failed before its own join)
    if (ctx->src_pending || ctx->tgt_pending) {
        // ONE round trip for both clouds' partials (they sit in one device buffer)
        float *res = (float *) pinned_scratch(ctx, 2 * 8 * sizeof(float) * kBboxBlocks);
        if (!res) return WM_ERR_HIP;
        const size_t slot = 8 * (size_t) kBboxBlocks;
        if (ctx->src_pending && ctx->tgt_pending) {
            WM_TRY(fast_fetch(ctx, res, ctx->cloud_bbox.p, 2 * slot * sizeof(float)));
        } else if (ctx->src_pending) {
            WM_TRY(fast_fetch(ctx, res, ctx->cloud_bbox.p, 8 * sizeof(float) * ctx->src_bbox_blocks));
        } else {
            WM_TRY(fast_fetch(ctx, res + slot, ctx->cloud_bbox.as<float>() + slot,
                              8 * sizeof(float) * ctx->tgt_bbox_blocks));
        }
    }
    // Both results are in: the target's grid ladder is enqueued FIRST (main stream), the source's Morton
    // sort behind it on the side stream.  The preparation is bound by how fast the host can enqueue its
    // ~55 small launches, not by the device: with the target's chain (the longer one on the device:
    // ~250 us at 1M points) enqueued first, the device works through it while the host is still
    // enqueueing the sort (sort first: the target's chain could not start before the sort's last launch
    // had been issued -- ~100 us later).
    const bool sort_src = ctx->src_pending;
    size_t src_valid = 0;
    if (sort_src) {
        ctx->src_pending = false;
        const float *res = (const float *) ctx->h_scratch;
        finish_bbox(res, ctx->src_bbox_blocks, &ctx->src_bbox, &src_valid);
        if (ctx->trace)
            fprintf(stderr, "[wm] source: valid=%zu lo=(%g %g %g) hi=(%g %g %g)\n", src_valid, ctx->src_bbox.lo[0],
                    ctx->src_bbox.lo[1], ctx->src_bbox.lo[2], ctx->src_bbox.hi[0], ctx->src_bbox.hi[1],
                    ctx->src_bbox.hi[2]);
    }
    const bool tgt_new = ctx->tgt_pending;
    if (tgt_new) {
        ctx->tgt_pending = false;
        const float *res = (const float *) ctx->h_scratch + 8 * (size_t) kBboxBlocks;
        size_t valid = 0;
        finish_bbox(res, ctx->tgt_bbox_blocks, &ctx->tgt_bbox, &valid);
        ctx->n_tgt = valid;
    }
    if (sort_src) ctx->n_src = src_valid;  // (the count of finite points: what the sort will leave in src_sorted)
    hipStream_t main_stream = ctx->stream;
    // the Morton sort of the source is independent of the target's grid build: side stream
    const bool aside = sort_aside != 0 && sort_src && ctx->side_stream != nullptr;
    const bool side = aside || (sort_src && ctx->side_stream && tgt_new && max_corr > 0);
    if (side) {  // (the sort may start as soon as what is on the main stream NOW -- the packed clouds -- is done)
        WM_HIP(ctx, hipEventRecord(ctx->ev_fork, main_stream));
        WM_HIP(ctx, hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    }
    int rc = WM_OK;
    if (max_corr > 0 && ctx->n_src > 0 && ctx->n_tgt > 0 && !use_brute(ctx, nn_method)) rc = ensure_levels(ctx, max_corr);
    if (sort_src && aside && sort_aside == 2) {
        ctx->sort_deferred = true;  // (enqueue_deferred_sort: the caller's own chain goes to the main stream first)
        return rc;
    }
    if (sort_src) {
        if (side) ctx->stream = ctx->side_stream;
        const int rc2 = morton_sort(ctx, ctx->src_orig.as<float4>(), ctx->n_src_input, ctx->src_bbox, src_valid,
                                    ctx->src_sorted.as<float4>());
        ctx->stream = main_stream;
        if (rc2 != WM_OK) return rc2;
        WM_TRACE(ctx, "source: sorted");
        if (side) {
            WM_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->side_stream));
            if (aside)
                ctx->sort_join_pending = true;
            else
                WM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        }
    }
    return rc;
}

}  // namespace wm

using namespace wm;

// =============================================================== C ABI
extern "C" {

const char *wm_version(void) { return "wavematch-hip 0.1 (gfx950, HIP)"; }

const char *wm_strerror(int s) {
    switch (s) {
        case WM_OK: return "ok";
        case WM_NOT_CONVERGED: return "registration did not converge";
        case WM_TOO_FEW_CORRESPONDENCES: return "not enough correspondences";
        case WM_ERR_ARG: return "invalid argument";
        case WM_ERR_HIP: return "HIP runtime error (see wm_last_error)";
        case WM_ERR_RCCL: return "RCCL error (see wm_last_error)";
        case WM_ERR_STATE: return "call sequence error (missing source/target cloud)";
        case WM_ERR_NOMEM: return "out of memory";
        default: return "unknown status";
    }
}

const char *wm_last_error(const wm_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

// ---- options: every knob of a context, by wm_set_option's name and by the environment variable read at wm_ctx_create.
// An integer or a float field, the closed range [lo, hi] of accepted values, and:
//   kOpenLo    the range is (lo, hi]
//   kFlag      any non-zero value means 1 -- except the top of the range, which is kept (gicp_served's 2)
//   kNdtModel  the NDT voxel model depends on it and is rebuilt
//   kOrZero    0 is accepted besides the range: back to the library's own choice
namespace {
enum : unsigned { kOpenLo = 1u, kFlag = 2u, kNdtModel = 4u, kOrZero = 8u };
struct Option {
    const char *name, *env;
    int wm_ctx::*i;
    float wm_ctx::*f;
    double lo, hi;
    unsigned flags;
};
constexpr double kIntMin = -2147483648.0, kIntMax = 2147483647.0, kFloatMax = 3.0e38;
const Option kOptions[] = {
    // the grid search (wm_nn.hip; the certificate kernel that shares its steps: wm_nn_cert.hip)
    {"lane_lf", "WM_TUNE_LANE_LF", nullptr, &wm_ctx::tune_lane_lf, 0, kFloatMax, kOpenLo},
    {"coop_lf", "WM_TUNE_COOP_LF", nullptr, &wm_ctx::tune_coop_lf, 0, kFloatMax, kOpenLo},
    {"r0", "WM_TUNE_R0", nullptr, &wm_ctx::tune_r0, 0, kFloatMax, kOpenLo},
    {"r_light", "WM_TUNE_R_LIGHT", nullptr, &wm_ctx::tune_r_light, 0, kFloatMax, kOpenLo},
    {"xcd_chunk", "WM_TUNE_XCD_CHUNK", &wm_ctx::tune_xcd_chunk, nullptr, kIntMin, kIntMax, 0},
    {"nn_balanced", "WM_TUNE_NN_BALANCED", &wm_ctx::tune_nn_balanced, nullptr, kIntMin, kIntMax, 0},
    // the ICP loop and its certificate kernel (wm_icp.hip)
    {"lag", "WM_TUNE_LAG", &wm_ctx::tune_lag, nullptr, 1, 16, 0},
    {"spin_us", "WM_TUNE_SPIN_US", &wm_ctx::tune_spin_us, nullptr, kIntMin, kIntMax, 0},
    {"cert_from", "WM_TUNE_CERT_FROM", &wm_ctx::tune_cert_from, nullptr, kIntMin, kIntMax, 0},
    {"cert_disp", "WM_TUNE_CERT_DISP", nullptr, &wm_ctx::tune_cert_disp, 0, kFloatMax, kOpenLo},
    {"cert_changed", "WM_TUNE_CERT_CHANGED", nullptr, &wm_ctx::tune_cert_changed, 0, kFloatMax, kOpenLo},
    {"cert_unsettled", "WM_TUNE_CERT_UNSETTLED", nullptr, &wm_ctx::tune_cert_unsettled, 0, kFloatMax, kOpenLo},
    {"cert_pad_mul", "WM_TUNE_CERT_PAD_MUL", nullptr, &wm_ctx::tune_cert_pad_mul, 0, kFloatMax, 0},
    {"cert_pad_frac", "WM_TUNE_CERT_PAD_FRAC", nullptr, &wm_ctx::tune_cert_pad_frac, 0, kFloatMax, 0},
    {"late", "WM_TUNE_LATE", &wm_ctx::tune_late, nullptr, kIntMin, kIntMax, kFlag},
    {"bins", "WM_TUNE_BINS", &wm_ctx::tune_bins, nullptr, kIntMin, kIntMax, 0},
    {"early_source", "WM_TUNE_EARLY_SOURCE", &wm_ctx::tune_early_source, nullptr, kIntMin, kIntMax, 0},
    {"shard_force", "WM_SHARD_FORCE", &wm_ctx::tune_force_shard, nullptr, kIntMin, kIntMax, 0},
    {"trace", "WM_TRACE", &wm_ctx::trace, nullptr, kIntMin, kIntMax, kFlag},
    // GICP (wm_gicp.hip)
    {"gicp_served", "WM_TUNE_GICP_SERVED", &wm_ctx::tune_gicp_served, nullptr, kIntMin, 2, kFlag},
    {"gicp_serve_test_stall_ms", "WM_TUNE_GICP_SERVE_TEST_STALL_MS", &wm_ctx::gicp_serve_test_stall_ms, nullptr, kIntMin, kIntMax, 0},
    {"gicp_blocks", "WM_TUNE_GICP_BLOCKS", &wm_ctx::tune_gicp_blocks, nullptr, 1, 4096, 0},
    {"knn_r0", "WM_TUNE_KNN_R0", nullptr, &wm_ctx::tune_knn_r0, 0.25, 8, kOrZero},
    {"gicp_profile", "WM_GICP_PROFILE", &wm_ctx::gicp_profile, nullptr, kIntMin, kIntMax, kFlag},
    // outlier removal (wm_outlier.hip)
    {"outlier_cell_div", "WM_TUNE_OUTLIER_CELL_DIV", nullptr, &wm_ctx::tune_outlier_cell_div, 0.5, 8, 0},
    // cluster extraction (wm_cluster.hip)
    {"cluster_cell_div", "WM_TUNE_CLUSTER_CELL_DIV", nullptr, &wm_ctx::tune_cluster_cell_div, 0.5, 8, 0},
    // plane segmentation (wm_sac.hip)
    {"sac_round", "WM_TUNE_SAC_ROUND", &wm_ctx::tune_sac_round, nullptr, 1, 1024, 0},
    // pose from correspondences (wm_corr_ransac.hip)
    {"corr_round", "WM_TUNE_CORR_ROUND", &wm_ctx::tune_corr_round, nullptr, 1, 1024, 0},
    // keypoints (wm_iss.hip)
    {"iss_cell_div", "WM_TUNE_ISS_CELL_DIV", nullptr, &wm_ctx::tune_iss_cell_div, 0.5, 8, 0},
    // radius normals and descriptors (wm_fpfh_radius.hip)
    {"fpfh_cell_div", "WM_TUNE_FPFH_CELL_DIV", nullptr, &wm_ctx::tune_fpfh_cell_div, 0.5, 8, 0},
    // sorting (wm_sort.hpp) and NDT (wm_ndt.hip)
    {"radix_min", "WM_TUNE_RADIX_MIN", &wm_ctx::tune_radix_min, nullptr, kIntMin, kIntMax, 0},
    // the grids' counting sort (wm_grid.hip)
    {"grid_rows", "WM_TUNE_GRID_ROWS", &wm_ctx::tune_grid_rows, nullptr, 0, 2, 0},
    {"ndt_dense", "WM_TUNE_NDT_DENSE", &wm_ctx::tune_ndt_dense, nullptr, kIntMin, kIntMax, 0},
    {"ndt_vox_split", "WM_TUNE_NDT_VOX_SPLIT", &wm_ctx::tune_ndt_vox_split, nullptr, kIntMin, kIntMax, kNdtModel},
    {"ndt_keys64", "WM_TUNE_NDT_KEYS64", &wm_ctx::tune_ndt_keys64, nullptr, kIntMin, kIntMax, kFlag | kNdtModel},
    {"ndt_blocks", "WM_TUNE_NDT_BLOCKS", &wm_ctx::tune_ndt_blocks, nullptr, 0, 4096, 0},
    {"ndt_spec_hessian", "WM_TUNE_NDT_SPEC_HESSIAN", &wm_ctx::tune_ndt_spec_hessian, nullptr, kIntMin, kIntMax, 0},
    {"ndt_fused_fetch", "WM_TUNE_NDT_FUSED_FETCH", &wm_ctx::tune_ndt_fused_fetch, nullptr, kIntMin, kIntMax, 0},
    {"ndt_profile", "WM_NDT_PROFILE", &wm_ctx::ndt_profile, nullptr, kIntMin, kIntMax, kFlag},
};

int apply_option(wm_ctx *ctx, const Option &o, double v) {
    if ((o.flags & kFlag) && v != o.hi) v = v != 0 ? 1 : 0;
    if ((!(v >= o.lo && v <= o.hi) || ((o.flags & kOpenLo) && v == o.lo)) && !((o.flags & kOrZero) && v == 0)) return WM_ERR_ARG;
    if (o.i) ctx->*o.i = (int) v;
    else ctx->*o.f = (float) v;
    if (o.flags & kNdtModel) ctx->ndt_built = false;
    return WM_OK;
}
}  // namespace

int wm_set_option(wm_ctx *ctx, const char *name, double value) {
    if (!ctx || !name) return WM_ERR_ARG;
    for (const Option &o : kOptions)
        if (strcmp(name, o.name) == 0) return apply_option(ctx, o, value);
    return WM_ERR_ARG;
}

int wm_ctx_create(wm_ctx **out, int device) {
    if (!out) return WM_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return WM_ERR_HIP;
    wm_ctx *ctx = new (std::nothrow) wm_ctx();
    if (!ctx) return WM_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&ctx->ev_a) != hipSuccess || hipEventCreate(&ctx->ev_b) != hipSuccess) {
        delete ctx;
        return WM_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    for (const Option &o : kOptions)
        if (const char *e = getenv(o.env)) (void) apply_option(ctx, o, atof(e));  // (a value out of range is ignored)
    // developer instrumentation, armed from the environment only
    if (const char *e = getenv("WM_LATE_DEBUG")) ctx->late_debug_iter = atoi(e) > 0 ? atoi(e) : 0;
    if (getenv("WM_CERT_PROF")) ctx->cert_prof_on = true;
    if (const char *e = getenv("WM_GICP_TRACE")) ctx->gicp_trace_path = e;
    if (getenv("WM_GICP_SERVE_DEBUG")) ctx->gicp_serve_debug = true;
    if (const char *e = getenv("WM_GICP_SMALL_TRACE")) ctx->gicp_small_trace = atoi(e);
    *out = ctx;
    return WM_OK;
}

int wm_ctx_set_stream(wm_ctx *ctx, void *hip_stream, int external) {
    if (!ctx) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    WM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // NB: a NULL handle with external != 0 is the (legacy) default stream -- which is
    // what torch.cuda.current_stream().cuda_stream returns unless a side stream is active
    ctx->stream = external ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return WM_OK;
}

void wm_ctx_destroy(wm_ctx *ctx) {
    if (!ctx) return;
    (void) hipSetDevice(ctx->device);
    if (ctx->stream) (void) hipStreamSynchronize(ctx->stream);
    DevBuf *bufs[] = {&ctx->src_sorted, &ctx->tgt_orig, &ctx->staging, &ctx->staging2, &ctx->cell_of, &ctx->counts,
                      &ctx->block_sums, &ctx->bbox_buf, &ctx->cloud_bbox, &ctx->keys, &ctx->keys_bak, &ctx->match_pt, &ctx->match_pt_bak, &ctx->d_levels, &ctx->ndt_keys, &ctx->ndt_keys2,
                      &ctx->ndt_vox, &ctx->ndt_vkey, &ctx->ndt_hkeys, &ctx->ndt_hvals, &ctx->ndt_dense, &ctx->ndt_meanf, &ctx->src_orig,
                      &ctx->gicp_c1, &ctx->gicp_c2, &ctx->gicp_mahal, &ctx->gicp_mailbox, &ctx->src_grid.pts,
                      &ctx->src_grid.cell_start, &ctx->vg_idx, &ctx->vg_idx2, &ctx->vg_perm,
                      &ctx->vg_perm2, &ctx->vg_tmp, &ctx->vg_seg, &ctx->io_a, &ctx->io_b, &ctx->ds_ref,
                      &ctx->ds_tgt, &ctx->match_ref, &ctx->match_tgt,
                      &ctx->partials, &ctx->partials2, &ctx->bins, &ctx->nn_bound, &ctx->late_ctl, &ctx->cert_count, &ctx->cert_prof, &ctx->cost_log, &ctx->phase_log, &ctx->shard_ref, &ctx->shard_tgt,
                      &ctx->shard_ref_band, &ctx->shard_tgt_band, &ctx->shard_misc, &ctx->shard_flags, &ctx->shard_pos_t,
                      &ctx->shard_pos_s, &ctx->shard_stats, &ctx->ndt_sum_dev, &ctx->corr_tmp_idx, &ctx->corr_tmp_d2, &ctx->d_state,
                      &ctx->plane_nrm, &ctx->plane_nrm_src, &ctx->plane_bins, &ctx->reject_buf, &ctx->reject_tmp,
                      &ctx->row_hist, &ctx->row_tmp};
    for (DevBuf *b : bufs) b->release();
    ctx->icp_stage.release();
    ctx->gicp_stage.release();
    ctx->ndt_stage.release();
    batch_voxel_release(ctx);
    ground_release(ctx);
    outlier_release(ctx);
    cluster_release(ctx);
    sac_release(ctx);
    boxes_release(ctx);
    fpfh_release(ctx);
    corr_release(ctx);
    iss_release(ctx);
    fpfh_radius_release(ctx);
    for (auto &l : ctx->levels) {
        l.pts.release();
        l.cell_start.release();
    }
    if (ctx->h_state) (void) hipHostFree(ctx->h_state);
    if (ctx->h_gicp) (void) hipHostFree(ctx->h_gicp);
    if (ctx->h_gicp_slots) (void) hipHostFree(ctx->h_gicp_slots);
    if (ctx->h_ndt) (void) hipHostFree(ctx->h_ndt);
    if (ctx->h_sig) (void) hipHostFree(ctx->h_sig);
    if (ctx->h_pub) (void) hipHostFree(ctx->h_pub);
    if (ctx->h_late) (void) hipHostFree(ctx->h_late);
    if (ctx->ev_block) (void) hipEventDestroy(ctx->ev_block);
    if (ctx->h_scratch) (void) hipHostFree(ctx->h_scratch);
    for (hipEvent_t e : ctx->ev_pool) (void) hipEventDestroy(e);
    if (ctx->ev_a) (void) hipEventDestroy(ctx->ev_a);
    if (ctx->ev_b) (void) hipEventDestroy(ctx->ev_b);
    if (ctx->ev_fork) (void) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void) hipEventDestroy(ctx->ev_join);
    if (ctx->side_stream) (void) hipStreamDestroy(ctx->side_stream);
    if (ctx->own_stream) (void) hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int wm_set_grid_cell(wm_ctx *ctx, float grid_cell) {
    if (!ctx || !(grid_cell >= 0)) return WM_ERR_ARG;
    ctx->grid_cell_override = grid_cell;
    for (auto &l : ctx->levels) l.built = false;
    ctx->n_levels = 0;
    ctx->levels_max_corr = -1;
    return WM_OK;
}

int wm_cloud_sizes(const wm_ctx *ctx, size_t *n_source, size_t *n_target) {
    if (!ctx) return WM_ERR_ARG;
    if (ctx->src_pending || ctx->tgt_pending) {  // counts of finite points: the pending reductions' results
        wm_ctx *c = const_cast<wm_ctx *>(ctx);
        WM_HIP(c, hipSetDevice(c->device));
        WM_TRY(finalize_clouds(c));
    }
    if (n_source) *n_source = ctx->n_src;
    if (n_target) *n_target = ctx->n_tgt;
    return WM_OK;
}

int wm_set_source(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem) {
    if (!ctx || (n > 0 && !pts) || stride < 12 || (stride & 3) || n > 0x7FFFFFF0u) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    ctx->sort_deferred = false;  // (a sort of the cloud that is replaced here, never enqueued: dropped)
    WM_TRY(join_source_sort(ctx));  // (a sort left running aside by a call that ended early: it reads what is replaced here)
    ctx->have_corr = false;
    ctx->n_src_input = n;
    ctx->n_src = 0;
    ctx->src_pending = false;
    if (n == 0) return WM_OK;
    // pack (caller order, kept for GICP's k-NN covariances) and launch the bounding-box reduction;
    // the Morton order is produced by finalize_clouds once the box has been fetched
    ctx->gicp_cov_src_valid = false;
    WM_HIP(ctx, ctx->src_orig.reserve(n * sizeof(float4)));
    WM_HIP(ctx, ctx->src_sorted.reserve(n * sizeof(float4)));
    WM_HIP(ctx, ctx->cloud_bbox.reserve(2 * 8 * sizeof(float) * kBboxBlocks));
    if (ctx->trace) fprintf(stderr, "[wm] set_source: n=%zu stride=%zu mem=%d ptr=%p\n", n, stride, mem, pts);
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, ctx->src_orig.as<float4>(), 0, false, ctx->cloud_bbox.as<float>(), &ctx->src_bbox_blocks));
    WM_TRACE(ctx, "set_source: packed");
    ctx->src_pending = true;
    return WM_OK;
}

int wm_set_target(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem) {
    if (!ctx || (n > 0 && !pts) || stride < 12 || (stride & 3) || n > 0x7FFFFFF0u) return WM_ERR_ARG;
    WM_HIP(ctx, hipSetDevice(ctx->device));
    ctx->have_corr = false;
    ctx->ndt_built = false;
    ctx->gicp_cov_tgt_valid = false;
    ctx->plane_nrm_valid = false;
    ctx->n_tgt_input = n;
    ctx->n_tgt = 0;
    ctx->tgt_pending = false;
    for (auto &l : ctx->levels) l.built = false;
    ctx->n_levels = 0;
    ctx->levels_max_corr = -1;
    if (n == 0) return WM_OK;
    WM_HIP(ctx, ctx->tgt_orig.reserve(n * sizeof(float4)));
    WM_HIP(ctx, ctx->cloud_bbox.reserve(2 * 8 * sizeof(float) * kBboxBlocks));
    int slot = 0;
    bool staged = false;
    if (mem == WM_MEM_HOST && ctx->src_pending && ctx->tune_early_source) {
        // (pinned caller memory: the upload STARTS here, on a copy engine, and runs under the source's round trip and the
        // ~150 us this thread needs to enqueue the source's sort -- a blocking copy behind those, round 3's order, left the
        // device idle for the 0.2 ms of the copy: the sort's launches are issued faster than it could start)
        if (ctx->tune_early_source >= 2) staged = upload_begin_async(ctx, pts, n * stride);
    }
    // (whatever ends this call early: the copy engine has finished with the caller's memory before it returns)
    struct DrainCopy {
        wm_ctx *c;
        bool on;
        ~DrainCopy() {
            if (on) (void) hipStreamSynchronize(c->side_stream);
        }
    } drain_copy{ctx, staged};
    if (mem == WM_MEM_HOST && ctx->src_pending && ctx->tune_early_source) {
        // A HOST target right behind a new source: this cloud is about to spend ~0.25 ms per 16 MB on PCIe with
        // the device idle.  Everything the source still needs -- its bounding box (one short round trip), its
        // Morton sort and gather -- is put on the stream first and runs under the copy (own staging buffer, no
        // drain of the stream: pack_cloud slot 1).
        float *res = (float *) pinned_scratch(ctx, 2 * 8 * sizeof(float) * kBboxBlocks);
        if (!res) return WM_ERR_HIP;
        WM_TRY(fast_fetch(ctx, res, ctx->cloud_bbox.p, 8 * sizeof(float) * ctx->src_bbox_blocks));
        size_t src_valid = 0;
        finish_bbox(res, ctx->src_bbox_blocks, &ctx->src_bbox, &src_valid);
        ctx->src_pending = false;
        ctx->n_src = src_valid;
        WM_TRY(morton_sort(ctx, ctx->src_orig.as<float4>(), ctx->n_src_input, ctx->src_bbox, src_valid,
                           ctx->src_sorted.as<float4>()));
        slot = 1;
    }
    WM_TRY(pack_cloud(ctx, pts, n, stride, mem, ctx->tgt_orig.as<float4>(), slot, staged, ctx->cloud_bbox.as<float>() + 8 * kBboxBlocks,
                      &ctx->tgt_bbox_blocks));
    drain_copy.on = false;  // (pack_cloud waited for it)
    ctx->tgt_pending = true;
    // the search grid is built by the first caller that searches (finalize_clouds / ensure_levels in
    // the ICP / GICP / search entry points): an NDT registration never needs it
    return WM_OK;
}

}  // extern "C"
