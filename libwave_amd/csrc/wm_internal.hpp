// wm_internal.hpp -- context, device-side structs and helpers shared by the
// HIP translation units of libwavematch_hip.so (gfx950 only).
#pragma once
#include <stdio.h>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/wavematch.h"
#include "wm_math.hpp"

namespace wm {

constexpr int kMaxLevels = 6;
constexpr int kBlock = 256;
constexpr unsigned kNoIdx = 0xFFFFFFFFu;
// all-reduced block of the sharded loop: the public WM_STATS_LEN slots + [kStatsLen]: queries the certificate
// kernel searched on this rank (summed: every rank steers by the same share) + one spare
constexpr int kBlkLen = 34;
constexpr int kAcc = 18;  // ICP statistics per partial row: 17 sums + the number of source points this rank handled

// ----------------------------------------------------------- error handling
#define WM_HIP(ctx, call)                                                              \
    do {                                                                               \
        hipError_t _e = (call);                                                        \
        if (_e != hipSuccess) {                                                        \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(_e);     \
            return WM_ERR_HIP;                                                         \
        }                                                                              \
    } while (0)

#define WM_TRY(expr)                \
    do {                            \
        int _s = (expr);            \
        if (_s != WM_OK) return _s; \
    } while (0)

// ----------------------------------------------------------- device buffers
// Growable device allocation cached on the context (hipMalloc is far too slow
// to sit inside match()).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void) hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
};

// The same for pinned host memory (hipHostMalloc): grows, never shrinks.
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void) hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const {
        return reinterpret_cast<T *>(p);
    }
};

inline size_t align_up256(size_t v) { return (v + 255) & ~(size_t) 255; }

// ---------------------------------------------- staging of the batched paths
// (wm_small.hip, wm_gicp_small.hip, wm_ndt_small.hip, wm_batch.hip; the functions: wm_stage.hpp)
// Hands out 256-byte aligned pieces of a block one after the other.  Without a block it only counts:
// a path states its pairs' scratch layout once, as calls of take(), and runs it twice.
struct Carver {
    unsigned char *base = nullptr;
    size_t used = 0;
    template <class T>
    T *take(size_t bytes) {
        unsigned char *p = base ? base + used : nullptr;
        used += align_up256(bytes);
        return reinterpret_cast<T *>(p);
    }
};

// A batch's clouds on their way to the kernels.  Host memory: copied into a pinned mirror back to back
// and sent in slices of 2 MB, so that each slice's DMA runs under the next copies; device memory: taken
// where it is.  The first `head` bytes are the caller's (a table it fills meanwhile and sends last).
struct SliceUpload {
    DevBuf dev;
    PinnedBuf host;
    size_t off = 0, sent = 0;
    bool host_clouds = false;
    // room for the batch; the caller waits for the stream (it may still read the mirror) before the first add()
    inline int begin(wm_ctx *ctx, size_t head, size_t cloud_bytes, int mem);
    inline int add(wm_ctx *ctx, const void *pts, size_t bytes, const unsigned char **on_device);  // -> the address a kernel shall read
    inline int flush(wm_ctx *ctx);  // sends what is still pending
    void release() {
        dev.release();
        host.release();
    }
};

struct PairJob {  // one registration of a batch: its clouds in the caller's layout, host or device memory
    const void *src;
    size_t n_src;
    const void *tgt;
    size_t n_tgt;
};

// One batch of registrations, a workgroup each: [table | host clouds] up, the pairs' scratch, the outputs back.
struct PairStage {
    SliceUpload up;
    DevBuf d_work, d_out;
    PinnedBuf h_out;
    Carver work;  // of d_work
    size_t table_bytes = 0;
    // the buffers, the wait for the stream (it may still read the mirror of the previous batch), the cursors
    inline int begin(wm_ctx *ctx, size_t table_bytes_, size_t cloud_bytes, size_t work_bytes, size_t out_bytes, int mem);
    template <class T>
    T *table() const {  // the host mirror, rows in the caller's order
        return up.host.as<T>();
    }
    template <class T>
    const T *d_table() const {
        return up.dev.as<const T>();
    }
    inline int submit(wm_ctx *ctx);  // the clouds' tail, then the table, then ev_a: the caller launches next
    inline int collect(wm_ctx *ctx, size_t out_bytes, float *kernel_ms);  // ev_b, the outputs into h_out, the wait
    void release() {
        up.release();
        d_work.release();
        d_out.release();
        h_out.release();
    }
};

// ------------------------------------------------------------ uniform grid
// One level of the target index: points cell-sorted (x fastest) in HBM, so the
// three x-adjacent cells of a query's neighbourhood are ONE contiguous run.
struct GridDev {
    float ox, oy, oz;  // origin (min corner)
    float h, inv_h;    // cell size
    float slack;       // cell-unit safety margin for float cell assignment
    int nx, ny, nz;
    const float4 *pts;          // cell-sorted, .w = original index bits
    const uint32_t *cell_start; // nx*ny*nz + 1
};

// the level ladder as the search kernels read it: a kernel argument BY VALUE (340 bytes of the kernarg segment: depth, cell
// sizes and level 0 are there when the wave starts) and a copy in HBM for the look-up of a level chosen at run time
struct LevelsDev {
    GridDev g[kMaxLevels];
    int n;
};

struct GridLevel {
    GridDev d{};
    DevBuf pts, cell_start;
    uint64_t ncells = 0;
    bool built = false;
};

// ----------------------------------------------------- ICP state in HBM
// Lives in device memory so that a whole registration runs without the host
// in the loop; mirrored to pinned host memory when the host needs to look.
struct IcpDevState {
    // ---- what a search wave reads before it can start (k_nn_grid, k_nn_cert): ONE aligned run of 80 bytes at the head
    // of the struct, fetched by two wide scalar loads issued together (nn_state, wm_nn_scan.hpp) -- these words used to
    // sit up to 0x4b4 bytes apart, a scalar round trip each where the compiler did not merge them
    float Tf[12];   // float rows 0..2 of T (what the correspondence kernel applies)
    int done;
    int have_prev;  // keys[] hold the previous iteration's result (level prediction)
    // sharded registration: this rank handles the source points whose transformed x
    // lies in [slab_lo, slab_hi)
    int slab_on;
    float slab_lo, slab_hi;
    // the count of changed matches rides in the fraction of the handled-points sum (units of 2^-24, wm_nn_scan.hpp:
    // icp_terms); beyond 2^23 queries per context only every (changed_mask + 1)-th query is counted, so
    // that the fraction can never carry into the integer part, and the count is scaled back up here
    unsigned changed_mask;
    float step_disp;   // upper estimate of how far the last step moved the source points (metres)
    int iter;  // (not read by the searches: it fills the run to a multiple of 8 bytes)
    // ---- the rest, in no particular order
    double T[16];   // cumulative source->target
    float Tf_search[12];  // ... the last correspondence search ran under (set by the solve that consumed it): what the keys' d2 refer to
    double Tk[16];  // last incremental step
    double stats[kStatsLen];
    double mse, prev_mse;
    int converged, state, n_corr, max_iter, forced, mode;
    // every rank holds only the source points near its slab; the all-reduced count of
    // handled points must equal the cloud size in EVERY iteration, else a point fell
    // outside all bands and the registration has to be redone with full source clouds
    double expect_owned;    // > 0: the count to expect; < 0: it arrives in the all-reduced block (slot 30: the sum of
                            // the ranks' stripe_finite); 0: no check
    double stripe_finite;   // finite source points in this rank's 1 / world stripe of the (full) source cloud
    int owned_violations;
    double rot_thr, trans_thr, fit_eps;
    unsigned queue_count[kMaxLevels + 1];
    unsigned long long deferred_total;
    int svd_warm;      // warm-started SVD on (always 1)
    double svd_v[10];  // V of the last iteration's SVD (+ a valid flag): the next one starts from it
    unsigned long long dbg[8];  // developer: cycle stamps of the last solve kernel (wm_debug_solve_cycles)
    unsigned cert_unsettled[64];  // k_nn_cert: queries it had to search in this iteration (partial counts; zeroed by the solve)
    double local_handled;  // queries THIS rank handled in the last search (sharded: before the all-reduce)
    float frac_changed;    // fraction of the handled queries whose match changed in the last search
    float frac_unsettled;  // fraction the last certificate launch had to search (0 after a full search)
    float src_radius;  // half diagonal of the source cloud's bounding box (for step_disp)
    float src_centre[3];
    int uns_global;  // sharded: the count of searched queries came through the all-reduced block (all ranks steer alike)
    int xchg_failed;  // sharded, in-kernel exchange (wm_xchg.hpp): a peer's block never arrived; the registration ended there
    // correspondence rejection (wm_reject.hip): the last executed iteration's matched count and threshold bits, copied
    // here by the kernel that ends a rejecting loop (k_reject_mark); 0 otherwise
    int n_matched, reject_bits;
    int pad_;
};
constexpr unsigned kNnStateWords = 20;  // the head run, in 32-bit words
static_assert(offsetof(IcpDevState, Tf) == 0 && offsetof(IcpDevState, done) == 48 && offsetof(IcpDevState, have_prev) == 52 &&
                  offsetof(IcpDevState, slab_on) == 56 && offsetof(IcpDevState, slab_lo) == 60 &&
                  offsetof(IcpDevState, slab_hi) == 64 && offsetof(IcpDevState, changed_mask) == 68 &&
                  offsetof(IcpDevState, step_disp) == 72 && offsetof(IcpDevState, T) == 4 * kNnStateWords,
              "the search kernels' head run of the state (nn_state, wm_nn_scan.hpp)");

struct Bbox {
    float lo[3], hi[3];
};

}  // namespace wm

// The opaque C handle.
struct wm_ctx {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    hipStream_t side_stream = nullptr;      // the source's Morton sort runs here, beside the target's grid build
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // wm_set_source / wm_set_target only pack the cloud and LAUNCH its bounding-box reduction; the
    // host fetches both results in one round trip when the first consumer needs them (finalize_clouds)
    bool src_pending = false, tgt_pending = false;
    unsigned src_bbox_blocks = 0, tgt_bbox_blocks = 0;
    wm::DevBuf cloud_bbox;                  // [2][kBboxBlocks][8] floats: source slot, target slot
    unsigned tuned_uses = 0;                // level-0 builds that trusted the cached cell size since the last check
    std::string last_error;

    // source (wave `ref`): Morton-ordered float4, .w = caller's index
    size_t n_src = 0, n_src_input = 0;
    wm::DevBuf src_sorted;

    // target (wave `target`)
    size_t n_tgt = 0, n_tgt_input = 0;
    wm::DevBuf tgt_orig;  // float4 in caller order, .w = index; non-finite -> NaN
    wm::Bbox tgt_bbox{};
    wm::GridLevel levels[wm::kMaxLevels];
    int n_levels = 0;
    double levels_max_corr = -1;
    float grid_cell_override = 0;
    // ---- options (wm_ctx.hip: kOptions names each one for wm_set_option and for the environment)
    int trace = 0;               // WM_TRACE: progress lines on stderr
    // the grid search (wm_nn.hip)
    float tune_lane_lf = 0.2f;   // lane-serial scan: finest level with cell size >= this x radius
    float tune_coop_lf = 0.5f;   // cooperative scan: finest level with cell size >= this x radius
    float tune_r0 = 0.5f;        // first radius of an unseeded search, in level-0 cells
    float tune_r_light = 16.0f;  // lane-serial vs cooperative scan threshold, in level-0 cells (12-24 within 1 %)
    int tune_xcd_chunk = 32;     // search kernel: XCDs take turns in chunks of this many workgroups (0: one eighth each)
    int tune_nn_balanced = 1;    // search kernel: wave-pooled candidate trips (0: every lane walks its own)
    // the ICP loop
    int tune_lag = 2;            // iterations the host may run ahead of the device (icp_run_loop), 1 ... 16
    int tune_spin_us = 80;       // host_wait: busy-poll this long before polling with yields
    int tune_bins = 1;           // 0: rows of partial sums + k_reduce_rows + k_reduce_solve, as up to round 5
    int tune_early_source = 2;   // a host target's upload overlaps the source's sort (wm_set_target); 2: and, from
                                 // pinned memory, starts on a copy engine before that sort is enqueued
    int tune_force_shard = 0;    // WM_SHARD_FORCE=1: a one-rank RCCL group still runs the sharded loop (plumbing check)
    int tune_cert_from = -1;     // k_nn_cert from this iteration of an align on (-1: chosen from the step size, tune_cert_disp; -2: never)
    float tune_cert_disp = 0.15f;  // ... once a step moves the points by less than this many level-0 cells
    float tune_cert_changed = 0.05f;   // ... AND fewer than this fraction of the matches changed in the last full search
    float tune_cert_unsettled = 0.40f; // back to full searches when a certificate launch had to search more than this fraction
    float tune_cert_pad_mul = 8.f, tune_cert_pad_frac = 0.5f;  // runner-up room of a certified search (see k_nn_cert)
    // 1: the late iterations run inside the resident kernel.  OFF by default: measured at 1M points
    // (profiles/r04_experiments.md) an iteration inside costs 33-43 us against 32-37 us for a launched certificate
    // iteration + its solve kernel -- the workers' certificate phase is bound by the vector ALU (~8 us chip-wide for the
    // f64 sums of a million queries), the slowest workgroup's searches end 10 us after the median one's, and the
    // solver's chain (rows 3.8, solve 4.4, hand-out 0.7 us) is serial behind them
    int tune_late = 0;
    // GICP (wm_gicp.hip)
    int tune_gicp_served = 1;    // 0: a kernel launch per evaluation; 1: resident evaluator; 2: ... without the on-chip copy of the pairs
    int gicp_serve_test_stall_ms = 0;  // test hook: the host sleeps this long before its third served evaluation
    int tune_gicp_blocks = 256;  // workgroups (= partial rows) of one GICP objective evaluation (double-double sums: 512 / 256 / 128 / 64 -> 6.9 / 6.4 / 7.3 / 9.6 ms per 500k registration)
    float tune_knn_r0 = 0.f;     // first radius of the k-NN (covariance) scan in cells, 0.25 ... 8; 0 = by k (1.0 up to k = 12, else 1.5)
    int gicp_profile = 0;        // HIP events around every objective evaluation (fdf_kernel_ms)
    // outlier removal (wm_outlier.hip)
    float tune_outlier_cell_div = 2.f;  // the radius filter's grid cell is at least radius / this (0.5 ... 8)
    // cluster extraction (wm_cluster.hip)
    float tune_cluster_cell_div = 2.f;  // the clustering's grid cell is at least tolerance / this (0.5 ... 8)
    // plane segmentation (wm_sac.hip)
    int tune_sac_round = 256;    // stream entries a round of the RANSAC loop evaluates at the most (1 ... 1024)
    // pose from correspondences (wm_corr_ransac.hip)
    int tune_corr_round = 256;   // the same for the RANSAC over correspondences (1 ... 1024)
    // keypoints (wm_iss.hip)
    float tune_iss_cell_div = 2.f;  // the detector's grid cell is at least max(salient, non-max radius) / this (0.5 ... 8)
    // radius normals and descriptors (wm_fpfh_radius.hip)
    float tune_fpfh_cell_div = 2.f;  // the call's grid cell is at least max(normal, feature radius) / this (0.5 ... 8)
    // sorting (wm_sort.hpp) and NDT (wm_ndt.hip)
    int tune_radix_min = 256 << 10;  // sorts of more items take the library's own radix sort, smaller ones rocPRIM's
    int tune_grid_rows = 1;      // a grid level's counting sort by (y, z) rows: 1 where it pays (rows_apply, wm_grid.hip), 0 never, 2 wherever possible
    int tune_ndt_dense = 2;      // 0: hash grid; 1: dense cell -> slot table; 2: + the float4 cell lattice
    int tune_ndt_vox_split = -1; // developer: points per voxel up to which a LANE forms a voxel's sums (-1: ndt_build's choice)
    int tune_ndt_keys64 = 0;     // developer: 64-bit voxel sort keys whatever the lattice's size
    int tune_ndt_blocks = 0;     // workgroups (= partial rows) of one NDT derivative pass; 0: one resident round
    int tune_ndt_spec_hessian = 1;  // form the Hessian along with the first extra line-search trial (step_length_mt)
    int tune_ndt_fused_fetch = 1;   // a pass's last workgroup adds the rows and hands the sums to the host
    int ndt_profile = 0;         // HIP events around every derivative pass (kernel_ms)
    // developer instrumentation, armed by environment variables at wm_ctx_create only
    int late_debug_iter = -1;    // WM_LATE_DEBUG: the resident kernel's stamps, its workers' of this iteration (-1: off)
    bool cert_prof_on = false;   // WM_CERT_PROF: wm_debug_cert_log also arms the certificate kernel's phase stamps
    std::string gicp_trace_path; // WM_GICP_TRACE: every GICP objective evaluation goes to this file
    bool gicp_serve_debug = false;  // WM_GICP_SERVE_DEBUG: device-side stamps of the served evaluator's first rounds
    int gicp_small_trace = 0;    // WM_GICP_SMALL_TRACE: the batched small GICP's trace (wm_gicp_small.hip)

    double tuned_h = 0, tuned_vol = 0;  // last auto-tuned level-0 cell size and its cloud
    size_t tuned_n = 0;
    double tuned_src_h = 0, tuned_src_vol = 0;  // the same for the source grid of the GICP covariances
    unsigned tuned_src_uses = 0;               // builds that trusted it since the last occupancy check
    size_t tuned_src_n = 0;

    // scratch
    wm::DevBuf staging, staging2, cell_of, counts, block_sums, bbox_buf;
    // the row-wise counting sort (wm_grid.hip): the tiles' counts per band of rows (+ the bands' totals and first
    // slots), the points ordered by band
    wm::DevBuf row_hist, row_tmp;
    wm::DevBuf match_pt, match_pt_bak;  // float4 per (sorted) source point: its match's xyz
    wm::PairStage icp_stage, gicp_stage, ndt_stage;  // staging of the batched small registrations (wm_small.hip, wm_gicp_small.hip, wm_ndt_small.hip)
    void *batch_voxel = nullptr;            // wm_batch.hip: buffers of the batched voxel filter
    void *ground = nullptr;                 // wm_ground.hip: the ground filter's workspace (its own, shared with nothing)
    void *outlier = nullptr;                // wm_outlier.hip: the outlier filters' workspace (its own as well)
    void *cluster = nullptr;                // wm_cluster.hip: the cluster extraction's workspace (its own as well)
    void *sac = nullptr;                    // wm_sac.hip: the plane segmentation's workspace (its own as well)
    void *boxes = nullptr;                  // wm_describe.hip: the cluster boxes' workspace (its own as well)
    void *fpfh = nullptr;                   // wm_fpfh.hip, wm_feature_match.hip: the descriptors' workspace (its own as well)
    void *corr = nullptr;                   // wm_corr_ransac.hip: the workspace of the RANSAC over correspondences (its own as well)
    void *iss = nullptr;                    // wm_iss.hip: the keypoint detector's workspace (its own as well)
    void *fpfh_radius = nullptr;            // wm_fpfh_radius.hip: the radius normals' and descriptors' workspace (its own as well)
    wm::DevBuf phase_log;                   // developer: per-iteration phase cycle sums of the search kernel
    wm::DevBuf cost_log;                    // developer: per-query search cost of every iteration (wm_debug_cost_log)
    int cost_log_iter = 0, cost_log_cap = 0;
    wm::DevBuf keys, partials, partials2, corr_tmp_idx, corr_tmp_d2, d_levels;
    wm::LevelsDev levels_dev{};  // the ladder as ensure_levels last published it (= d_levels): what a search launch passes by value
    // the iteration's sums as exact integer limbs (wm_bins.hpp): all zero between iterations (the solve puts the
    // zeros back)
    wm::DevBuf bins;
    bool bins_dirty = false;     // an iteration loop is running or ended abnormally: the bins may hold sums
    wm::DevBuf nn_bound;                    // float4 per (sorted) source point, written by k_nn_cert's searches: where the query was (xyz) and a lower bound (w) on its distance, there, to every target point but its match
    wm::DevBuf cert_count;                  // developer: unsettled queries per launch of k_nn_cert ([launch][64] partial counts)
    wm::DevBuf cert_prof;                   // developer: phase cycle sums per launch of k_nn_cert ([launch][8][8])
    int cert_log_iter = 0, cert_log_cap = 0;
    int cert_launches = 0;                  // of the last align
    // the resident late-iteration kernel (k_nn_cert<.., LATE>)
    int late_capacity = 0;                  // workgroups of it the device holds at once (0: not asked yet, -1: unusable)
    wm::DevBuf late_ctl;                    // LateCtl
    unsigned long long *h_late = nullptr;   // pinned: its exit word
    unsigned late_seq = 0;
    int late_iters = 0, late_launches = 0;  // of the last align: iterations that ran inside it
    float late_ms = 0.f;                    // ... and its event-timed duration (profile >= 1)
    unsigned long long *h_pub = nullptr;    // pinned: [0] (done << 63 | iterations finished << 32 | step size bits) of the latest solve, [k] iteration k's own record
    int h_pub_slots = 0;
    wm::DevBuf vg_idx, vg_idx2, vg_perm, vg_perm2, vg_tmp, vg_seg, io_a, io_b, ds_ref, ds_tgt, match_ref, match_tgt;
    wm::DevBuf d_state;
    wm::IcpDevState *h_state = nullptr;  // pinned
    void *h_scratch = nullptr;           // pinned, device-visible scratch (reduction partials, level table)
    size_t h_scratch_bytes = 0;
    unsigned *h_sig = nullptr;           // pinned: completion flag polled by fast_fetch
    unsigned sig_seq = 0;
    // served GICP evaluations (wm_gicp.hip): the mailbox in device memory the host writes through the BAR
    wm::DevBuf gicp_mailbox;
    unsigned gicp_serve_seq = 0;
    unsigned gicp_serve_abandoned = 0;      // rounds after which the evaluator's `abandoned` word was found set (diagnostic)
    int gicp_serve_ok = 0, gicp_serve_capacity = 0, gicp_serve_cached = 0;  // 0: not tried yet, 1: usable, -1: not on this system
    void *h_gicp_slots = nullptr;         // pinned: the evaluator's answers, thirteen (sum, command number) pairs
    double *h_gicp = nullptr;            // pinned, device-visible: the GICP objective's partial sums land here
    int ndt_rank = 0, ndt_world = 1;     // wm_ndt_set_shard: this context's slice of the source
    int (*ndt_reduce)(double *, int, void *) = nullptr;
    void *ndt_reduce_user = nullptr;
    double *h_ndt = nullptr;             // pinned: the NDT derivative passes' block partials
    bool have_corr = false, last_align_valid = false, last_align_converged = false;
    bool last_align_sharded = false;     // the last align was this rank's part of a sharded registration (wm_icp_info_sharded)
    wm::DevBuf keys_bak;
    double corr_T[16];

    // carried PCL object state
    double prev_mse = -1;

    // events for profile mode
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    hipEvent_t ev_block = nullptr;  // the event sync_sleeping polls between short sleeps
    std::vector<float> iter_nn_ms;

    // GICP: caller-order source, its own search grid, per-point covariances
    wm::DevBuf src_orig, gicp_c1, gicp_c2, gicp_mahal;
    wm::Bbox src_bbox{};
    wm::GridLevel src_grid;
    bool gicp_cov_src_valid = false, gicp_cov_tgt_valid = false;
    int gicp_cov_k = 0;
    double gicp_cov_eps = 0;

    // point-to-plane ICP (wm_plane.hip): the target's normals (float4 nx ny nz curvature, caller order), valid until the
    // target changes; the source's of the last wm_estimate_normals; the plane pass's own bins (29 components)
    wm::DevBuf plane_nrm, plane_nrm_src, plane_bins;
    bool plane_nrm_valid = false;
    int plane_nrm_k = 0;

    // correspondence rejection (wm_reject.hip): the select's histograms, tickets and record; scratch of the two
    // developer entry points (keys built from floats, the kept mask)
    wm::DevBuf reject_buf, reject_tmp;

    // NDT voxel model of the target
    wm::DevBuf ndt_keys, ndt_keys2, ndt_vox, ndt_vkey, ndt_hkeys, ndt_hvals, ndt_dense, ndt_meanf, ndt_vsum;
    bool ndt_dense_on = false;  // dense cell -> voxel-slot table built (small lattices)
    int ndt_dense_lo[3] = {0, 0, 0}, ndt_dense_dim[3] = {0, 0, 0};
    int ndt_lat_lo[3] = {0, 0, 0}, ndt_lat_dim[3] = {1, 1, 1};  // the voxel lattice over the target: low corner (cells), cells per axis
    bool ndt_cells4_on = false;
    wm::DevBuf ndt_cells4;
    int ndt_cus = 0;
    wm::DevBuf ndt_ticket;
    wm::DevBuf ndt_perm, ndt_perm2, ndt_flags, ndt_seg, ndt_tmp;  // ndt_build's scratch (its own: see there)
    bool xchg_timed_out = false;  // the last sharded loop ended because a peer's block did not arrive (wm_shard.hip)
    bool sort_join_pending = false;  // the source's Morton sort runs on the side stream, ev_join recorded, nobody waits yet
    bool sort_deferred = false;      // ... is still to be enqueued there (finalize_clouds mode 2: ev_fork recorded, n_src = the finite points' count)
    unsigned ndt_seq = 0;
    bool ndt_built = false;
    int ndt_model_builds = 0;    // voxel models built so far (wm_ndt_stats.model_builds)
    double ndt_res = -1;
    unsigned ndt_nvox = 0, ndt_nvalid = 0, ndt_hmask = 0;

    // sharded (multi-GPU) stepping
    wm::DevBuf shard_ref, shard_tgt, shard_ref_band, shard_tgt_band, shard_misc, shard_flags, shard_flags2, shard_pos_t,
        shard_pos_s, shard_stats, ndt_sum_dev;
    float shard_lo = 0, shard_hi = 0;
    struct wm_comm *ndt_comm = nullptr;    // wm_ndt_set_comm: the derivative passes' sums are all-reduced on the device
    bool shard_active = false;
    wm_icp_params shard_params{};
    float shard_thr = 0;
    bool shard_brute = false;
};

namespace wm {

// developer tracing (env WM_TRACE=1): drain the stream and print a marker, so that a GPU fault can
// be pinned to the stage that was running
#define WM_TRACE(ctx, what)                                                     \
    do {                                                                        \
        if ((ctx)->trace) {                                                     \
            (void) hipStreamSynchronize((ctx)->stream);                         \
            fprintf(stderr, "[wm] %s\n", what);                                 \
            fflush(stderr);                                                     \
        }                                                                       \
    } while (0)

// ---- host-side waits for a word the device writes into pinned memory
// one turn of a host-side busy-wait (the pause hint of the host's architecture; nothing where there is none)
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}
// Wait until arrived() holds, in three stages.  Spin (most waits are tens of microseconds); then, after tune_spin_us,
// poll with a yield between looks, so that worker threads sharing a core take turns instead of starving each other
// (kernels of a few hundred microseconds: the NDT passes at 2M points); only after `block_after` let the runtime
// block in hipStreamSynchronize -- its wake-up costs 0.1-0.2 ms on some hosts, which a registration that waits a
// hundred times cannot afford, but it is the right thing for a wait of milliseconds and it is what reports a failed
// kernel.  The clock is looked at every 64th spin, and between yields.
// kWaitArrived: arrived() held; kWaitBlocked: everything enqueued has run, and the caller looks again (what it waits
// for is there, unless a kernel ended without writing it); kWaitFailed: the runtime reported an error (last_error).
enum HostWait { kWaitArrived, kWaitBlocked, kWaitFailed };
template <class Pred>
inline HostWait host_wait(wm_ctx *ctx, Pred arrived, std::chrono::milliseconds block_after) {
    const auto t0 = std::chrono::steady_clock::now();
    bool yielding = false;
    for (unsigned spins = 1; !arrived(); ++spins) {
        if (yielding)
            std::this_thread::yield();
        else
            cpu_relax();
        if ((spins & 63u) == 0 || yielding) {
            const auto waited = std::chrono::steady_clock::now() - t0;
            if (waited > block_after) {
                const hipError_t e = hipStreamSynchronize(ctx->stream);
                if (e == hipSuccess) return kWaitBlocked;
                ctx->last_error = std::string("hipStreamSynchronize(ctx->stream): ") + hipGetErrorString(e);
                return kWaitFailed;
            }
            yielding = waited > std::chrono::microseconds(ctx->tune_spin_us);
        }
    }
    return kWaitArrived;
}

// ---- wm_ctx.hip
// Fetch what wm_set_source / wm_set_target left pending (bounding boxes, finite-point counts), then
// Morton-sort the source on the side stream while -- when max_corr > 0 and the search will use the
// grid -- the target's level ladder is built on the main stream; both are joined before returning.
// sort_aside: the source's Morton sort goes to the side stream and the call does NOT wait for it (ctx->sort_join_pending;
// join_source_sort makes the context's stream wait) -- for a caller with work of its own to enqueue meanwhile
// sort_aside = 2: ... and the sort is not even ENQUEUED yet (ctx->sort_deferred): the caller enqueues what is on its own
// critical path first and calls enqueue_deferred_sort when it comes to its first wait for the device (wm_ndt_align)
int finalize_clouds(wm_ctx *ctx, double max_corr = -1.0, int nn_method = 0, int sort_aside = 0);
int join_source_sort(wm_ctx *ctx);
int enqueue_deferred_sort(wm_ctx *ctx);
int prepare_work(wm_ctx *ctx);  // keys, match points, partial rows and the iteration state for the source's size
bool use_brute(const wm_ctx *ctx, int nn_method);  // all-pairs instead of the grid (WM_NN_AUTO: by the clouds' sizes)
hipEvent_t get_event(wm_ctx *ctx, size_t k);       // event k of the context's pool (profile mode)
// one correspondence pass with transform T; `predict` lets the search start from the
// radii in the current keys
int nn_pass(wm_ctx *ctx, const double T[16], float thr_d2, double max_corr, bool predict, bool slab = false,
            float slab_lo = 0.f, float slab_hi = 0.f, bool wait = true);

// ---- wm_fetch.hip
// fetch a small result from device memory into pinned host memory and wait for it (copy, fence
// and completion flag by one wavefront; see k_fetch_signal)
int fast_fetch(wm_ctx *ctx, void *dst_pinned, const void *src_dev, size_t bytes);
// column sums of a [rows][k] f64 block (k <= 32), reduced on the device, k doubles delivered
int fast_fetch_sum(wm_ctx *ctx, double *dst_pinned, const double *src_dev, unsigned rows, unsigned k);
// a caller-supplied producer kernel that ends with fast_fetch's fence + flag protocol (it gets the
// flag's address and the sequence number to write); waits for it
int fast_fetch_begin(wm_ctx *ctx, unsigned **flag, unsigned *seq);
int fast_fetch_wait(wm_ctx *ctx, unsigned seq);
// results that a kernel hands over as 16-byte slots {double value, unsigned number, 0} in pinned memory, one store each
// (no flag behind the data, hence no system-scope fence): wait until all n slots carry `seq`
int wait_slots(wm_ctx *ctx, const double *slots, int n, unsigned seq);
template <class Launch>
inline int fast_fetch_custom(wm_ctx *ctx, Launch launch) {
    unsigned *flag = nullptr, seq = 0;
    WM_TRY(fast_fetch_begin(ctx, &flag, &seq));
    launch(flag, seq);
    WM_HIP(ctx, hipGetLastError());
    return fast_fetch_wait(ctx, seq);
}
// the same column sums left in DEVICE memory (no signal): what an all-reduce then works on
int sum_to_device(wm_ctx *ctx, double *dst_dev, const double *src_dev, unsigned rows, unsigned k);
// pinned, device-visible host scratch of at least `bytes` (kernels write small results into it
// through fast_fetch; the host reads them once its flag has arrived)
void *pinned_scratch(wm_ctx *ctx, size_t bytes);
// device -> caller (pageable) memory: drain the stream, then a blocking copy (the caller's pages
// are pinned and unpinned by the runtime inside that one call)
int copy_to_caller(wm_ctx *ctx, void *dst, const void *src_dev, size_t bytes);
// Wait for everything enqueued on the context's stream WITHOUT burning a core: the batched paths wait
// milliseconds per launch, and a crew of MultiMatcher workers that all spin through their waits
// (hipStreamSynchronize busy-polls) exhausts a container's CPU quota -- the whole process is then
// throttled, staging threads included.  The thread sleeps between looks at an event (wake-up ~0.1 ms).
int sync_sleeping(wm_ctx *ctx);

// ---- wm_grid.hip
// (bbox_partials / bbox_blocks: the packed cloud's bounding-box partials as launch_bbox leaves them, in the same launch)
int pack_cloud(wm_ctx *ctx, const void *pts, size_t n, size_t stride, int mem, float4 *out, int slot = 0, bool staged = false,
               float *bbox_partials = nullptr, unsigned *bbox_blocks = nullptr);
bool upload_begin_async(wm_ctx *ctx, const void *pts, size_t bytes);  // (pinned host memory: the copy starts now, see wm_grid.hip)
int compute_bbox(wm_ctx *ctx, const float4 *pts, size_t n, Bbox *out, size_t *n_valid);
// the two halves of compute_bbox: enqueue the reduction into `partials_dev` (kBboxBlocks * 8 floats),
// and finish it on the host from the fetched partials
constexpr int kBboxBlocks = 512;
int launch_bbox(wm_ctx *ctx, const float4 *pts, size_t n, float *partials_dev, unsigned *blocks_out);
void finish_bbox(const float *partials_host, unsigned blocks, Bbox *out, size_t *n_valid);
int build_grid_level(wm_ctx *ctx, const float4 *pts, size_t n, const Bbox &bb, float h,
                     GridLevel *lvl, double *avg_occupancy);
// one call's grid over an arbitrary packed cloud: the automatic cell, never below floor_h (see wm_grid.hip)
int build_call_grid(wm_ctx *ctx, const float4 *pts, size_t n, size_t n_finite, const Bbox &bb, float floor_h,
                    GridLevel *grid);
int morton_sort(wm_ctx *ctx, const float4 *pts, size_t n, const Bbox &bb, size_t n_valid,
                float4 *out);
int ensure_levels(wm_ctx *ctx, double max_corr);
int exclusive_scan(wm_ctx *ctx, const unsigned *in, size_t n, unsigned *out);

// ---- wm_shard.hip: sum `n` doubles in device memory over the ranks of `comm`, on the context's stream
int comm_allreduce(wm_ctx *ctx, struct wm_comm *comm, double *dev, int n);
struct XchgDev;
// WM_OK (and *out filled) when the communicator has mailboxes for the in-kernel exchange of the sharded loop's block
int comm_exchange_args(struct wm_comm *comm, XchgDev *out);

// ---- wm_voxel.hip
// pcl::VoxelGrid on device: `in` is a packed float4 cloud (w = index, NaN = invalid);
// writes centroids (float4, w = output index) to `out` (capacity >= n), count to *n_out
// `known`: the cloud's bounding box and finite-point count if the caller already has them (the
// multiscale match filters the same cloud at four leaf sizes); nullptr = computed here
struct VgKnown {
    Bbox bb;
    size_t valid;
};
int voxel_downsample_dev(wm_ctx *ctx, const float4 *in, size_t n, float leaf, float4 *out,
                         size_t *n_out, const VgKnown *known = nullptr);
int transform_cloud_dev(wm_ctx *ctx, const float4 *in, size_t n, const double T[16], float4 *out);

// ---- wm_nn.hip (the full search, brute force), wm_nn_cert.hip (the certificate kernel, launched and resident)
// stats_mode < 0: search only; WM_ICP_SVD / WM_ICP_GN6: the search kernel also reduces the ICP
// statistics of the iteration to *rows_out rows of kAcc doubles in ctx->partials
int launch_nn_grid(wm_ctx *ctx, float thr_d2, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2,
                   int stats_mode = -1, unsigned *rows_out = nullptr, bool use_bins = false);
int launch_nn_brute(wm_ctx *ctx, float thr_d2, hipEvent_t ev0, hipEvent_t ev1);
// where a search kernel's sums go: the iteration's bins (*bins) or `blocks` rows of ctx->partials (*rows_out)
int nn_sums_target(wm_ctx *ctx, int stats_mode, bool use_bins, unsigned blocks, long long **bins, unsigned *rows_out);
// the resident form of the certificate kernel (wm_nn_cert.hip: k_nn_cert<.., LATE>): the late iterations in one launch
bool late_possible(wm_ctx *ctx, int stats_mode, unsigned *blocks_out);
size_t late_ctl_bytes();  // sizeof(LateCtl): the developer stamps sit behind it
int launch_nn_late(wm_ctx *ctx, float thr_d2, int stats_mode, unsigned blocks, bool bounds_valid, unsigned exit_seq,
                   float stop_unsettled, float stop_disp, int max_inside);
// the device's budget of resident workgroups (per process), in 1/1024ths of the device: the share taken (0: refused)
int resident_admit(int device, int nb, int capacity);
void resident_release(int device, int share);
int launch_fix_keys(wm_ctx *ctx, float thr_d2);  // after certified iterations: every key's distance brought up to date
// the certificate kernel (late iterations): stats_mode as above; bounds_valid = the previous search of
// this align was launch_nn_cert too (its per-query bounds are still in ctx->nn_bound)
int launch_nn_cert(wm_ctx *ctx, float thr_d2, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2, int stats_mode,
                   unsigned *rows_out, bool bounds_valid, bool use_bins = false);
float threshold_d2(double max_corr);
float threshold_d2_strict(double max_corr);

// ---- wm_small.hip: whole registrations inside one workgroup, many per launch
struct SmallJob {
    const void *src;
    size_t n_src;
    const void *tgt;
    size_t n_tgt;
    double prev_mse0;
    int presorted;  // the source is already in a spatial order (skips the in-kernel sort)
};
struct SmallResult {
    double T[16];
    double info[36];
    double mse, prev_mse;
    int iterations, converged, state, n_corr, info_degenerate;
    float cell;
    unsigned long long cyc[4];
};
int small_run(wm_ctx *ctx, const SmallJob *jobs, int n, size_t stride, int mem, const wm_icp_params *p, int with_info,
              double info_max_corr, SmallResult *res, float *kernel_ms);
void small_fill_stats(const SmallResult &r, float kernel_ms, wm_icp_stats *s);

// ---- wm_batch.hip
// pcl::VoxelGrid of all the clouds of a batch in one pass (see there)
int batch_voxel_filter(wm_ctx *ctx, const wm_batch_item *items, const std::vector<int> &idx, size_t stride, int mem, float leaf,
                       const float4 **filtered, std::vector<unsigned> &off, std::vector<unsigned> &n_out);
void batch_voxel_release(wm_ctx *ctx);
int batch_match_scaled(wm_ctx *ctx, const wm_batch_item *items, int n_items, size_t stride, int mem,
                       const wm_icp_params *p, float res, int multiscale_steps, int with_info, double *T_out,
                       double *info_out, wm_icp_stats *stats, int *status);

// ---- wm_ground.hip
void ground_release(wm_ctx *ctx);

// ---- wm_outlier.hip
void outlier_release(wm_ctx *ctx);

// ---- wm_cluster.hip
void cluster_release(wm_ctx *ctx);

// ---- wm_sac.hip
void sac_release(wm_ctx *ctx);

// ---- wm_describe.hip
void boxes_release(wm_ctx *ctx);

// ---- wm_fpfh.hip (the workspace both descriptor files share; wm_feature_match.hip's part is released with it)
void fpfh_release(wm_ctx *ctx);

// ---- wm_corr_ransac.hip
void corr_release(wm_ctx *ctx);

// ---- wm_iss.hip
void iss_release(wm_ctx *ctx);

// ---- wm_fpfh_radius.hip
void fpfh_radius_release(wm_ctx *ctx);

// ---- wm_plane.hip: the point-to-plane metric (WM_ICP_PLANE)
constexpr int kPlaneDefaultK = 20;  // neighbours of a normal when the caller says 0
int plane_normal_k(int k);          // 0 -> the default
int plane_target_normals(wm_ctx *ctx, int k);  // the target's normals on the context (cached per target and k)
// the source's on ctx->plane_nrm_src (its grid stays on ctx->src_grid); k resolved
int plane_source_normals(wm_ctx *ctx, int k, bool grid_ready = false);
int plane_bins_ready(wm_ctx *ctx);
int launch_plane_stats(wm_ctx *ctx, const int *rej = nullptr);  // after a search-only launch: the 29 sums into the plane bins
int launch_plane_solve(wm_ctx *ctx, unsigned long long *pub, int pub_slots, int solve);  // solve == 0: the sums into st->stats only

// ---- wm_reject.hip: correspondence rejection (wm_icp_params.reject)
bool reject_params_ok(int reject, double ratio, double factor, int min_corr);  // the valid ranges of wavematch.h
int reject_ready(wm_ctx *ctx);  // the select's histograms and tickets: allocated and all zero
// the threshold of the keys' matched pairs under the rule (WM_REJECT_*; -1: the element of rank `rank`), left on the
// device: three histogram passes; returns at once on st->done
int launch_reject_select(wm_ctx *ctx, const unsigned long long *keys, unsigned n, int rule, double ratio, double factor,
                         unsigned min_corr, unsigned rank);
const int *reject_threshold(const wm_ctx *ctx);  // where that threshold's bit pattern is (what the filtered sums read)
int launch_reject_mark(wm_ctx *ctx);  // behind a loop's last iteration: rejected keys lose their index, the record -> the state
// the statistics kernels (wm_icp.hip, wm_plane.hip) with the filter: rej = reject_threshold(ctx) or nullptr
int launch_stats(wm_ctx *ctx, int mode, const int *rej = nullptr);
unsigned stat_rows(const wm_ctx *ctx);  // rows of partial sums launch_stats leaves
int launch_sum_rows(wm_ctx *ctx);       // ... added up into st->stats (no solve)

// ---- wm_gicp.hip
int source_grid(wm_ctx *ctx);  // the source's own search grid (ctx->src_grid), built over src_orig

// ---- wm_icp.hip
void init_state(IcpDevState *s, const double *T, const wm_icp_params *p, double prev_mse);  // p == nullptr: a search's state
int upload_state(wm_ctx *ctx);  // ctx->h_state -> the device
int bins_ready(wm_ctx *ctx);    // the iteration's bins (wm_bins.hpp) allocated and all zero
int shard_begin(wm_ctx *ctx, const wm_icp_params *p, double x_lo, double x_hi, double expect, double stripe_finite,
                bool *brute_out, float *thr_out, double prev_mse0);
// the iteration loop of one registration (state already uploaded); blk != nullptr: sharded (see wm_icp.hip)
int icp_run_loop(wm_ctx *ctx, const wm_icp_params *p, bool brute, float thr, struct wm_comm *comm, double *blk,
                 double T_out[16], wm_icp_stats *stats);

// ---- wm_debug.hip
// developer (WM_LATE_DEBUG): the resident ICP kernel's stamps after a launch that ran `inside` iterations
void late_debug_report(wm_ctx *ctx, unsigned late_blocks, int inside, int reason);

}  // namespace wm
