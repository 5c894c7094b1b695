/*
 * wavematch.h -- C ABI of libwavematch_hip.so: the MI355X (gfx950) registration
 * back end behind libwave's wave::Matcher<PCLPointCloudPtr> API.
 *
 * The reference (wavelab/libwave) has no FFI boundary on this path: its
 * ICPMatcher / GICPMatcher / NDTMatcher call PCL C++ templates directly.  Each
 * entry point below names the reference call (file:line under /root/reference)
 * whose work it replaces; the C++ shim in include/wave/matching maps the
 * reference's classes onto these calls.
 *
 * Conventions
 *   - every function returns an int status: 0 = WM_OK, >0 = algorithmic
 *     "no result" (the reference's match() == false), <0 = error.  No C++
 *     exceptions cross this boundary.
 *   - clouds are arrays of points with a caller-given byte stride whose first
 *     12 bytes are float x, y, z (pcl::PointXYZ is stride 16; packed XYZ is 12).
 *     `mem` says where the array lives: WM_MEM_HOST (copied H2D by the call) or
 *     WM_MEM_DEVICE (an HBM pointer, e.g. a torch tensor's data_ptr()).
 *     The library never retains a caller pointer past the call.
 *   - 4x4 transforms and 6x6 matrices are row-major doubles.
 *   - a wm_ctx is thread-compatible (one thread at a time); distinct contexts
 *     are fully concurrent (own HIP stream).  One ctx == one reference matcher
 *     object (it carries PCL's per-object state, e.g. the convergence
 *     criteria's previous MSE).
 */
#ifndef WAVEMATCH_H
#define WAVEMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM_OK 0
#define WM_NOT_CONVERGED 1            /* pcl hasConverged() == false */
#define WM_TOO_FEW_CORRESPONDENCES 2  /* PCL: "Not enough correspondences found" */
#define WM_ERR_ARG (-1)
#define WM_ERR_HIP (-2)
#define WM_ERR_RCCL (-3)
#define WM_ERR_STATE (-4) /* e.g. align before set_source/set_target */
#define WM_ERR_NOMEM (-5)

enum { WM_MEM_HOST = 0, WM_MEM_DEVICE = 1 };

typedef struct wm_ctx wm_ctx;

/* ------------------------------------------------------------- lifecycle */
/* Replaces the PCL member objects a matcher constructs (icp.hpp:100-102,
 * gicp.hpp:61-62, ndt.hpp:72).  `device` is the HIP device ordinal. */
int wm_ctx_create(wm_ctx **out, int device);
void wm_ctx_destroy(wm_ctx *ctx);
const char *wm_strerror(int status);
/* last HIP/RCCL error text recorded on this ctx ("" if none) */
const char *wm_last_error(const wm_ctx *ctx);
/* library / build identification, e.g. "wavematch-hip 0.1 gfx950" */
const char *wm_version(void);

/* external != 0: adopt the caller's HIP stream (e.g. torch's current stream, so that
 * collectives issued by the caller order correctly against this context's kernels);
 * a NULL handle then means the default stream.  external == 0: back to the context's
 * own stream.  The external stream is not owned. */
int wm_ctx_set_stream(wm_ctx *ctx, void *hip_stream, int external);

/* ---------------------------------------------------------------- clouds */
/* wave `ref` == PCL source (the cloud that is moved / queried):
 *   icp.setInputSource  wave_matching/src/icp.cpp:87,110,125
 *   gicp.setInputSource wave_matching/src/gicp.cpp:44
 *   ndt.setInputSource  wave_matching/src/ndt.cpp:50
 * Uploads, drops non-finite points, and Morton-orders the cloud in HBM. */
int wm_set_source(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem);
/* wave `target` == PCL target (the cloud that is indexed):
 *   icp.setInputTarget  wave_matching/src/icp.cpp:91,114,124
 *   gicp.setInputTarget wave_matching/src/gicp.cpp:54
 *   ndt.setInputTarget  wave_matching/src/ndt.cpp:55
 * Replaces the FLANN kd-tree build in pcl::Registration::initCompute with a
 * cell-sorted uniform grid in HBM.  grid_cell = 0 picks the cell size from the
 * measured point density. */
int wm_set_target(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem);
int wm_set_grid_cell(wm_ctx *ctx, float grid_cell);
/* number of points currently held (after dropping non-finite ones) */
int wm_cloud_sizes(const wm_ctx *ctx, size_t *n_source, size_t *n_target);

/* ------------------------------------------------------------------- ICP */
enum { WM_ICP_SVD = 0, WM_ICP_GN6 = 1,
       /* point-to-plane: the residual n . (p - q) with q's normal n (pcl::IterativeClosestPointWithNormals /
        * TransformationEstimationPointToPlaneLLS; libwave's ICPMatcher has no counterpart: an opt-in) */
       WM_ICP_PLANE = 2 };
enum { WM_NN_AUTO = 0, WM_NN_GRID = 1, WM_NN_BRUTE = 2,
       /* wm_nn_search only, OR-ed in: seed every query with the point it matched in the previous
        * search of the same clouds (what consecutive ICP iterations do); same result, less work */
       WM_NN_WARM = 0x100 };
enum { /* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
       WM_CONV_NOT_CONVERGED = 0,
       WM_CONV_ITERATIONS = 1,
       WM_CONV_TRANSFORM = 2,
       WM_CONV_ABS_MSE = 3,
       WM_CONV_REL_MSE = 4,
       WM_CONV_NO_CORRESPONDENCES = 5,
       WM_CONV_FORCED = 6,
       /* WM_ICP_PLANE and WM_ICP_GN6 (no PCL counterpart): J^T J of an iteration is singular to rounding.  PLANE: the
        * matched normals leave a motion free (one plane: three).  GN6: the matched pairs do -- collinear pairs (a line
        * against a line, three pairs in a row) the rotation about their line, coincident ones every rotation; a
        * Cholesky pivot at or below 1e-12 of its own diagonal entry says so, on every path (wm_icp_align, wm_icp_match,
        * wm_icp_batch_match, the sharded ones, wm_host_icp_apply; wm_gn6_from_stats returns WM_NOT_CONVERGED).  The
        * align ends NOT converged, T_out untouched: loud, not wrong -- the step of such a system was measured to
        * raise the residual by many orders of magnitude.  WM_ICP_SVD is well defined on the same input (any of the
        * equally good rotations) and registers it */
       WM_CONV_DEGENERATE = 7 };
/* Correspondence rejection between an iteration's search and its step (pcl::IterativeClosestPoint::
 * addCorrespondenceRejector with ONE rejector) [PCL-upstream: restated from PCL 1.8's registration/impl/icp.hpp,
 * correspondence_rejection_trimmed.cpp and correspondence_rejection_median_distance.cpp; no PCL on the build machine].
 * Per iteration: C = the matched queries (finite source points with a neighbour inside max_corr), n = |C|, d2_i = the
 * search's own float squared distance (PCL's Correspondence::distance in ICP).
 *   WM_REJECT_TRIMMED (CorrespondenceRejectorTrimmed; PCL's defaults: ratio 0.5, min 0)
 *       k = max((unsigned) floor(reject_ratio * (double) n), reject_min_corr); k >= n: nothing is rejected; k == 0:
 *       everything is; else t = the k-th smallest d2 (1-based) and a pair is kept iff d2_i <= t.
 *       DEVIATION from PCL: PCL keeps exactly k pairs (nth_element), which of several pairs tied at the k-th place
 *       survive being unspecified; here ALL pairs tied at t are kept -- order-independent, kept count >= k.
 *   WM_REJECT_MEDIAN (CorrespondenceRejectorMedianDistance; PCL's default factor: 1.0)
 *       m = the element of 0-based rank n / 2 of the ascending d2; kept iff (double) d2_i <= (double) m * reject_factor.
 * The step, n_corr and the stopping rules' MSE are those of the kept pairs (PCL's rejectors rewrite correspondences_
 * before min_number_correspondences_, the estimation and the criteria see it); fewer than 3 kept pairs end the align
 * with WM_CONV_NO_CORRESPONDENCES.  After the align the context's correspondences are the kept pairs of the last
 * executed iteration (wm_get_correspondences: -1 for a rejected pair, its d2 stays; wm_icp_info's LUM / Censi work on
 * them).  The threshold is an exact order statistic found on the device (wm_reject.hip): bit-reproducible. */
enum { WM_REJECT_NONE = 0, WM_REJECT_TRIMMED = 1, WM_REJECT_MEDIAN = 2 };

typedef struct {
    double max_corr;      /* ICPMatcherParams::max_corr, icp.hpp:35 -> icp.cpp:47 */
    int max_iter;         /* ICPMatcherParams::max_iter, icp.hpp:37 -> icp.cpp:48 */
    double t_eps;         /* ICPMatcherParams::t_eps,    icp.hpp:41 -> icp.cpp:49 */
    double fit_eps;       /* ICPMatcherParams::fit_eps,  icp.hpp:43 -> icp.cpp:50 */
    int force_iterations; /* >0: run exactly this many iterations (bench; no stop tests) */
    int mode;             /* WM_ICP_SVD: PCL's Umeyama step (parity default).  Accuracy far from the origin: sigma is
                             formed from RAW sums (Sqp / n - qm pm^T), which costs seven to eight digits 55 km out --
                             measured there: one step within 2.3e-8 m of a centred long double Umeyama over the points
                             of a 30 m cloud (1.6e-9 rad, which is 9e-5 m of the pose's translation); near the origin
                             within 1e-13 m (tests/test_icp_stress_gpu.py);
                             WM_ICP_GN6: 6x6 J^T J / J^T r Gauss-Newton step, the rotation linearised about the
                             ORIGIN (far from it a first step overshoots by |dw|^2 |p| / 2); ends with
                             WM_CONV_DEGENERATE where the pairs leave a motion free;
                             WM_ICP_PLANE: the same 6x6 step on the point-to-plane residual, with normals
                             of the target estimated on the device once per target (wm_estimate_normals);
                             the stopping rules and their MSE (mean point-to-point d^2) are unchanged.
                             wm_icp_align, wm_icp_match and wm_icp_batch_match (every item through
                             wm_icp_match inside the call: correct, not fast) take it; the sharded entry
                             points (wm_icp_shard_*, wm_icp_*_sharded, wm_multi_*) return WM_ERR_ARG */
    int nn_method;        /* WM_NN_AUTO | WM_NN_GRID | WM_NN_BRUTE */
    int carry_state;      /* 1: seed the criteria's previous MSE from the ctx (PCL keeps
                             it across align() calls on one object); 0: fresh */
    int profile;          /* HIP-event timing on the ctx stream: 1 = the level-0
                             correspondence kernel only; 2 = every kernel class */
    int normal_k;         /* WM_ICP_PLANE: neighbours per normal, 3 ... 32; 0 = the default, 20 */
    int reject;           /* WM_REJECT_NONE (default) | WM_REJECT_TRIMMED | WM_REJECT_MEDIAN, every step mode.  A
                             rejecting align searches in full every iteration (no certificate kernel, no fused sums):
                             search, select (three histogram passes), filtered sums, solve.  wm_icp_align,
                             wm_icp_match (every align of every scale) and wm_icp_batch_match (every item through
                             wm_icp_match inside the call: correct, not fast) take it; the sharded entry points
                             (wm_icp_shard_*, wm_icp_*_sharded, wm_multi_*) return WM_ERR_ARG */
    double reject_ratio;  /* WM_REJECT_TRIMMED: the overlap ratio, finite in [0, 1]; default 0.5 */
    double reject_factor; /* WM_REJECT_MEDIAN: the factor on the median, finite and >= 0; default 1.0 */
    int reject_min_corr;  /* WM_REJECT_TRIMMED: keep at least this many pairs, >= 0; default 0 */
} wm_icp_params;

typedef struct {
    int converged;  /* hasConverged() */
    int iterations; /* nr_iterations_ */
    int state;      /* WM_CONV_* */
    int n_corr;     /* correspondences of the last iteration */
    double mse;     /* mean d^2 of the last iteration's correspondences */
    double prev_mse;
    /* measurement (HIP events on the ctx stream; ms) */
    float align_ms;      /* whole wm_icp_align call, device side */
    float nn_ms;         /* sum over level-0 correspondence-kernel launches (profile=1) */
    float coarse_ms;     /* sum over the coarser-level launches for deferred queries */
    float stats_ms;      /* sum over statistic-reduction launches (profile=1) */
    float solve_ms;      /* sum over reduce+solve launches (profile=1) */
    int nn_launches;     /* level-0 correspondence launches timed in nn_ms */
    int nn_levels;       /* grid levels used */
    uint64_t deferred;   /* queries that needed a coarser grid level (profile=1) */
    float grid_cell;     /* level-0 cell size used */
    int owned_violations; /* sharded path: iterations in which the ranks together did not
                             handle every source point (see wm_icp_shard_begin) */
    int cert_launches;   /* iterations whose correspondences came from the certificate kernel
                            (k_nn_cert: previous match proved still nearest, search only where the
                            proof fails) instead of a full search; same correspondences either way */
    float nn_cert_ms;    /* the part of nn_ms spent in those launches (profile >= 1) */
    /* sharded registrations (wm_icp_align_sharded): where this rank's time went, so that a multi-GPU
       run explains itself.  Device times from HIP events on the context's stream, ms. */
    float plan_ms;       /* x range + 64 Ki-bin histogram of a fixed sub-sample of the target, slab edges */
    float compact_ms;    /* this rank's target slab + halo and source band selected out of the full clouds */
    float index_ms;      /* host wall time: packing, bounding boxes, source order, grid ladder of the LOCAL clouds */
    float iter_ms;       /* host wall time of the iteration loop (search, sums, all-reduce, solve) */
    float allreduce_ms;  /* sum over the iterations' all-reduces of WM_STATS_LEN doubles (profile >= 1) */
    unsigned n_tgt_local, n_src_local; /* points this rank indexed / searched */
    int rccl_ranks;      /* ncclCommCount of the communicator (0: none or the in-process stand-in) */
    int shard_attempts;  /* 2 if the registration had to be redone with full source clouds */
    /* the resident late-iteration kernel (k_nn_cert<.., LATE>: certificate, searches, sums, solve and
       stopping rules of the late iterations in ONE launch; counted in cert_launches too) */
    int late_iterations; /* iterations that ran inside it */
    int late_launches;   /* its launches (1, unless its own policy sent it back to full searches in between) */
    float late_ms;       /* their duration by HIP events (profile >= 1): search + sums + solve of those iterations */
    int exchange_in_kernel; /* sharded: 1 if the iterations' blocks were exchanged through the ranks' mailboxes inside
                               the solve kernel (one launch per iteration's tail), 0 if by ncclAllReduce between two */
    int n_matched;       /* the last iteration's matched queries BEFORE rejection (== n_corr without rejection; n_corr
                            and mse stay what the step used: the kept pairs) */
    float reject_d2;     /* the last iteration's rejection threshold (kept iff d2 <= it); FLT_MAX: the rule kept
                            everything, -1: it rejected everything; 0 without rejection */
} wm_icp_stats;

void wm_icp_default_params(wm_icp_params *p);

/* pcl::IterativeClosestPoint::align + hasConverged + getFinalTransformation
 * (wave_matching/src/icp.cpp:95-101,116-119,126-129).  T_out maps source->target.
 * Returns WM_OK when converged, WM_NOT_CONVERGED / WM_TOO_FEW_CORRESPONDENCES
 * otherwise (T_out then untouched, as ICPMatcher leaves `result`). */
int wm_icp_align(wm_ctx *ctx, const wm_icp_params *p, double T_out[16], wm_icp_stats *stats);

/* ICPMatcher::match() in one call (wave_matching/src/icp.cpp:75-133): with both
 * caller clouds as inputs, runs the reference's three branches entirely on device
 *   res > 0 && multiscale_steps > 0 : for i = steps..0: leaf = 2^i * res, VoxelGrid
 *        both clouds, pre-transform the filtered ref by the running transform,
 *        max_corr = 2^i * p->max_corr, align, running = T_i * running  (icp.cpp:77-104)
 *   res > 0 && multiscale_steps == 0: VoxelGrid both clouds, align    (icp.cpp:105-122)
 *   res <= 0                         : align on the full clouds       (icp.cpp:123-131)
 * Returns WM_OK and writes T_out only when every align converged (as match() does). */
int wm_icp_match(wm_ctx *ctx, const void *ref, size_t n_ref, const void *target, size_t n_target,
                 size_t stride_bytes, int mem, const wm_icp_params *p, float res,
                 int multiscale_steps, double T_out[16], wm_icp_stats *stats);

/* Many registrations per launch -- the throughput path under wave::MultiMatcher
 * (wave_matching/include/wave/matching/multi_matcher.hpp:29-96; worker loop impl/
 * multi_matcher_impl.hpp:45-53: setRef, setTarget, match, estimateInfo per queued pair).  Every item
 * is ICPMatcher::match() as wm_icp_match runs it (res, multiscale_steps: the three branches of
 * icp.cpp:75-133), with stopping criteria that start fresh, and, with with_info = 1, the estimator
 * whose result estimateInfo() always ends with (icp.cpp:135-142 -> estimateLUMold,
 * icp_pcl_functions.cpp:51-179, on the clouds of the last align).  One workgroup per item runs a
 * whole align: a target of up to WM_BATCH_LDS_TARGET_POINTS points lives, cell-sorted, in its compute
 * unit's LDS; larger ones, up to WM_BATCH_MAX_TARGET_POINTS (16-bit slots and indices), in HBM scratch
 * that the L2 / Infinity Cache keep close (same code, ~3x slower per point).
 *   res <= 0: the clouds as given; a target beyond WM_BATCH_MAX_TARGET_POINTS is WM_ERR_ARG
 *             (register such pairs one by one).
 *   res > 0 : both clouds of every item go through pcl::VoxelGrid first -- all clouds of the batch in
 *             one pass of device-wide kernels, the cloud number above the leaf index in one sort key --
 *             per scale (leaf = 2^i res, i = multiscale_steps .. 0; icp.cpp:77-104) or once
 *             (multiscale_steps == 0; icp.cpp:105-122); an item that fails at a scale stops there, as
 *             match() does.  Items whose filtered target is still too large, or whose leaf lattice is
 *             beyond the batched filter (PCL's size rule fires: the product of the truncated extents
 *             overflows int32 and the cloud stays unfiltered; or the rule passes while the lattice
 *             itself has 2^32 cells or more), are registered by wm_icp_match inside the call.
 * Results per item k: status[k] (what wm_icp_match would have returned), T_out + 16 k (written
 * when status[k] == WM_OK), info_out + 36 k (with_info; written whenever an align of the item ran),
 * stats[k] (of the item's last align).  T_out, info_out, stats may be NULL.  The call returns WM_OK
 * when the batch ran.  In stats[k], align_ms is the device time of the launches the item took part
 * in; nn_ms / stats_ms / solve_ms / coarse_ms carry a developer aid instead of times: shader-clock
 * kilocycles of the item's LAST iteration (query loop, row sum, solve) and of its set-up. */
#define WM_BATCH_LDS_TARGET_POINTS 10000
#define WM_BATCH_MAX_TARGET_POINTS 65535
typedef struct {
    const void *src;    /* wave `ref`    */
    size_t n_src;
    const void *target; /* wave `target` */
    size_t n_target;
} wm_batch_item;
int wm_icp_batch_match(wm_ctx *ctx, const wm_batch_item *items, int n_items, size_t stride_bytes,
                       int mem, const wm_icp_params *p, float res, int multiscale_steps,
                       int with_info, double *T_out, double *info_out, wm_icp_stats *stats,
                       int *status);

/* pcl::VoxelGrid<PointXYZ>::filter of MANY clouds in one pass (the filter stage of wm_icp_batch_match
 * with res > 0, exposed): cloud 2 k = items[k].src, 2 k + 1 = items[k].target; their centroids, back
 * to back in that order, as packed xyz floats in host memory out_xyz (capacity cap_points points),
 * their counts in n_out[2 n_items].  Same results, bit for bit, as wm_voxel_downsample cloud by cloud
 * (a cloud for which PCL's size rule fires -- wm_voxel_downsample returns it unfiltered -- or whose
 * lattice has 2^32 cells or more is WM_ERR_ARG here). */
int wm_voxel_downsample_batch(wm_ctx *ctx, const wm_batch_item *items, int n_items, size_t stride_bytes,
                              int mem, float leaf, float *out_xyz, size_t cap_points, size_t *n_out);

/* pcl::VoxelGrid<PointXYZ>::filter on device (icp.cpp:81-90,106-113; gicp.cpp:39-40,
 * 49-50): float centroid per occupied leaf, ascending leaf index (PCL's `unsigned int` index:
 * mod 2^32 where the lattice has more cells); `out` must hold `cap` points of `out_stride` bytes. */
int wm_voxel_downsample(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                        float leaf, void *out, size_t out_stride, int out_mem, size_t cap,
                        size_t *n_out);

/* pcl::transformPointCloud(in, out, Eigen::Affine3d) on device (icp.cpp:84-86; every
 * reference test fixture, tests/icp_tests.cpp:31): double arithmetic, float store. */
int wm_transform_cloud(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                       const double T[16], void *out, size_t out_stride, int out_mem);

/* ICPMatcher's information-matrix estimators on the correspondences of the last
 * align (wave_matching/src/icp.cpp:135-142):
 *   WM_INFO_LUM     estimateLUM     icp_pcl_functions.cpp:182-289
 *   WM_INFO_CENSI   estimateCensi   icp.cpp:167-397   (T_result = Matcher::result,
 *                   lin/ang_covar = ICPMatcherParams::lidar_{lin,ang}_covar)
 *   WM_INFO_LUMOLD  estimateLUMold  icp_pcl_functions.cpp:51-179  (fresh exact NN of
 *                   the aligned cloud, d2 < max_corr^2)
 * info is the 6x6 row-major result.  *degenerate (may be NULL) is set when the LUM
 * residual s^2 underflows: LUM then yields identity, LUMold divides by it anyway
 * (both as the reference does).  LUM / Censi return WM_NOT_CONVERGED and leave info
 * untouched when the last align did not converge (the reference's hasConverged()
 * guard). */
enum { WM_INFO_LUM = 0, WM_INFO_CENSI = 1, WM_INFO_LUMOLD = 2 };
int wm_icp_info(wm_ctx *ctx, int method, const double T_result[16], double lin_covar,
                double ang_covar, double max_corr, double info[36], int *degenerate);

/* Device-to-device copy rate of this GPU (GB/s, read + write bytes) measured with a plain float4
 * copy kernel on the context's stream: the practical HBM ceiling to hold next to the 8 TB/s
 * specification (bench.py's roofline.peak_measured_copy). */
int wm_debug_copy_bandwidth(wm_ctx *ctx, size_t bytes, int reps, double *gb_per_s);
/* developer / tests, HOST ONLY (no device is touched): the arithmetic the ICP loop's sums go through on the device
 * (libwave_amd/csrc/wm_bins.hpp) -- every x[i] cut into three signed 40-bit limbs of trunc(x * 2^56), the limbs added as
 * 64-bit integers into 64 bins in the order perm[] names (NULL: as given), the totals turned back into one double.
 * *out = that double; limbs_out (may be NULL): the three limb totals.  WM_ERR_ARG when an x[i] does not fit (not finite,
 * |x| >= 2^62: the device poisons the bin for those). */
int wm_debug_bins_sum(const double *x, size_t n, const unsigned *perm, double *out, long long limbs_out[3]);
/* Developer / tests: the library's own stable radix sort (wm_sort.hpp: what every cloud's Morton order, the NDT voxel
 * order and the voxel filter are built on above 256k points) on HOST arrays: values_out[i] = the input position of the
 * i-th pair in ascending order of the low `bits` bits of the key (equal keys in input order).  key_bytes: 4 or 8. */
int wm_debug_sort_pairs(wm_ctx *ctx, const void *keys, int key_bytes, size_t n, unsigned bits, unsigned *values_out);
/* Developer / tests: the neighbour lists behind wm_gicp_covariances and wm_estimate_normals -- the k nearest points of
 * every point of the source (which = 0) or the target (which = 1) in its own cloud, the point itself included, found by
 * the same search on the same grid, along the same query route and from the same first radius (option "knn_r0") as
 * those two.  idx_out / d2_out: HOST arrays of n_input x k, rows and indices in the caller's order, a row ascending by
 * (float squared distance, index); -1 / 0 where a list is short and in the row of a non-finite point.  k: 1 ... 32.
 * WM_NOT_CONVERGED when the cloud has fewer than k finite points, WM_ERR_STATE without both clouds.  Cached covariances,
 * normals and tuned cell sizes stay as they were. */
int wm_debug_knn(wm_ctx *ctx, int which, int k, int32_t *idx_out, float *d2_out);
/* Developer / tests, synchronous: one level of the target's search grid as the search kernels read it.  max_corr > 0:
 * the ladder for that radius is built first if it is not there (no source needed); otherwise the level must exist
 * (WM_ERR_STATE).  geom[5] = origin x y z, cell size h, 1 / h; dims[3] = nx ny nz; *n_points = the points the level
 * holds (the finite ones).  cell_start (HOST, may be NULL): nx * ny * nz + 1 words when cell_cap holds them; pts (HOST,
 * may be NULL): *n_points + 4 entries of four floats (x y z, the original index's bits) -- the cell-sorted array and the
 * four pad entries behind it -- when pts_cap (in entries) holds them.  WM_ERR_ARG when a given buffer is too small
 * (geom, dims and *n_points are filled all the same: call once without buffers for the sizes). */
int wm_debug_grid_level(wm_ctx *ctx, int level, double max_corr, float geom[5], int dims[3], size_t *n_points,
                        unsigned *cell_start, size_t cell_cap, float *pts, size_t pts_cap);
/* Tuning knobs by name (tests, benchmarks; the defaults are the product's).  Each is also read from the environment
 * when a context is created (mostly WM_TUNE_<NAME>; INTEGRATION.md lists them all).  Among them: "cert_from"
 * (-1: the certificate kernel takes over once an ICP step is small, -2: never, k >= 0: from iteration k of every
 * align), "cert_disp" (that step size, in level-0 grid cells), "cert_pad_mul", "cert_pad_frac", "gicp_served"
 * (0 / 1 / 2: GICP's objective evaluations launched / served by the resident evaluator / served without the on-chip
 * pair cache), "late" (1: the late ICP iterations -- certificate, searches, sums, solve, stopping rules -- in ONE
 * resident launch, k_nn_cert<.., LATE> + k_late_solver; 0, the default: a launch per iteration, which measures the
 * same or faster), "bins" (0: an ICP iteration's sums as rows of partial sums and a reduction launch; 1, the default:
 * as exact integer limbs in bins), "ndt_vox_split" (NDT model: the points per voxel up to which a lane, not a wave,
 * forms a voxel's sums; -1: the library's choice) and "ndt_keys64" (1: 64-bit voxel sort keys whatever the lattice's
 * size) -- both rebuild the model at the next NDT call.  None of them changes a result.  WM_ERR_ARG for an unknown
 * name or a value outside the knob's range. */
int wm_set_option(wm_ctx *ctx, const char *name, double value);
/* developer: out == NULL arms a log of `iterations` launches (0 disarms); otherwise writes, per
 * launch of the certificate kernel since, how many queries it had to search; returns the count */
int wm_debug_cert_log(wm_ctx *ctx, int iterations, unsigned *out, int cap);
/* developer (armed by wm_debug_cert_log with WM_CERT_PROF set): 64 words per launch -- 16 cycle stamps
 * of each of four sampled workgroups (see k_nn_cert) */
int wm_debug_cert_prof(wm_ctx *ctx, unsigned long long *out, int cap);
/* developer: the per-iteration records the solve kernels of the last align published for the host
 * ([k], k >= 1: iteration : 16 | step size bfloat16 : 16 | changed matches : 16 | searched : 16) */
int wm_debug_pub_log(wm_ctx *ctx, unsigned long long *out, int cap);
/* Per-iteration device time (ms) of the correspondence kernel in the last
 * wm_icp_align call that ran with profile >= 1; returns the number written. */
int wm_get_iteration_times(wm_ctx *ctx, float *nn_ms, int cap);

/* Developer aid: shader-clock stamps of the last solve kernel of the last align (start, rows
 * added, statistics expanded, solve + stopping rules done). */
int wm_debug_solve_cycles(wm_ctx *ctx, unsigned long long out[8]);
/* Developer aid: per-query work of the grid search.  out == NULL arms the log for the first
 * `iterations` iterations of the next wm_icp_align on the current clouds (0 disarms and frees it);
 * out != NULL copies the log ([iteration][query in Morton order]: trips of the candidate loop in
 * bits 0-15, row chunks in bits 16-23, scan passes in bits 24-27 (saturating), rungs of the radius
 * probe of a query that had no candidate in bits 28-30 (saturating), bit 31 = handed to the
 * wave-cooperative path) and returns the number of iterations recorded. */
int wm_debug_cost_log(wm_ctx *ctx, int iterations, unsigned *out, size_t cap);
/* with the cost log armed: per iteration, shader-clock cycle sums over the waves of the search kernel's
 * phases -- out[8 k + 0..7] = walk, pooled rounds, walks, prologue, pass loop, cooperative phase + stores,
 * statistics tail, waves.  Returns the number of iterations copied. */
int wm_debug_phase_log(wm_ctx *ctx, unsigned long long *out, int iterations);

/* PCL's icp.correspondences_ after align (read by estimateLUM / estimateCensi,
 * icp_pcl_functions.cpp:191, icp.cpp:213): per source point (caller's order)
 * the matched target index (caller's order; -1 = none) and squared distance. */
int wm_get_correspondences(wm_ctx *ctx, int32_t *match_idx, float *d2, size_t cap);

/* One correspondence pass with a caller-given transform (kernel-level parity
 * and roofline measurement): CorrespondenceEstimation::determineCorrespondences
 * [PCL registration/impl/correspondence_estimation.hpp] as driven by
 * icp.align (icp.cpp:126).  kernel_ms (may be NULL) receives the device time
 * of the level-0 correspondence kernel. */
int wm_nn_search(wm_ctx *ctx, const double T[16], double max_corr, int nn_method,
                 int32_t *match_idx, float *d2, size_t cap, float *kernel_ms);

/* Normals of the context's target (which = 1) or source (which = 0), mirroring wm_gicp_covariances: per point the
 * k nearest points of the same cloud, the point itself included (the neighbourhood of computeCovariances, same tie
 * order: distance, then index), their covariance in double about the neighbourhood mean, the unit eigenvector of its
 * smallest eigenvalue turned towards the origin (pcl::flipNormalTowardsViewpoint with the viewpoint at 0: n . p <= 0)
 * and the curvature lambda0 / (lambda0 + lambda1 + lambda2) -- pcl::NormalEstimation with setKSearch(k).  normals_out:
 * float x 4 (nx, ny, nz, curvature) per input point in the caller's order, in host or device memory (`out_mem`).  A
 * non-finite point, or a neighbourhood whose largest eigenvalue is 0, gives (0, 0, 0, 0).  k: 3 ... 32, 0 = the
 * default, 20.  WM_NOT_CONVERGED when the cloud has fewer than k finite points.  The target's normals stay on the
 * context (what a WM_ICP_PLANE align with the same k uses) until the target changes. */
int wm_estimate_normals(wm_ctx *ctx, int which, int k, void *normals_out, int out_mem);

/* The sufficient statistics one ICP iteration reduces to (what crosses xGMI in
 * the multi-GPU path).  SVD mode: stats[0]=n, [1..3]=sum p, [4..6]=sum q,
 * [7..15]=sum q p^T (row-major), [16]=sum d2.  GN6 mode: [0]=n, [1]=sum d2,
 * [2..22]=upper triangle of J^T J (row-major), [23..28]=J^T r.  PLANE mode: the GN6 layout with the rows
 * J = [n^T, (p x n)^T] and r = n . (p - q) (n: the matched point's normal on the context -- those of the last plane
 * align or wm_estimate_normals, else estimated with the default k; a pair whose normal is zero adds to [0], [1] only).
 * All: [31] = number of
 * source points this context handled (== cloud size unless sharded).  Uses the
 * correspondences of the last wm_nn_search / align iteration. */
#define WM_STATS_LEN 32
int wm_icp_stats_for(wm_ctx *ctx, const double T[16], int mode, double stats[WM_STATS_LEN]);

/* Developer / tests: the element of 0-based rank `rank` of n HOST floats (bit patterns of non-negative floats), found by
 * the rejection's select kernels (wm_reject.hip).  WM_ERR_ARG unless rank < n < 2^31. */
int wm_debug_rank_select(wm_ctx *ctx, const float *vals, size_t n, size_t rank, float *out);

/* One iteration's rejection on the correspondences of the last search (wm_nn_search / an align), under pose T:
 * the threshold, the counts, the kept mask in the caller's order (n_source_input bytes; may be NULL) and the mode's sums
 * over the kept pairs (may be NULL; layout of wm_icp_stats_for).  reject = WM_REJECT_NONE keeps every matched pair.
 * all_kept: the rule kept everything whatever the distances (threshold_d2 = FLT_MAX); a rule that rejected everything
 * reports threshold_d2 = -1.  Leaves the context's correspondences as they are. */
typedef struct { int n_matched, n_kept; float threshold_d2; int all_kept; } wm_icp_reject_result;
int wm_icp_reject(wm_ctx *ctx, const double T[16], int mode, int reject, double ratio, double factor, int min_corr,
                  wm_icp_reject_result *res, unsigned char *kept_out, double stats_out[WM_STATS_LEN]);

/* Host-only solvers on those statistics (no GPU touched; used by every rank
 * after the all-reduce).  Tk_out is the incremental transform of one step:
 * TransformationEstimationSVD / pcl::umeyama [PCL transformation_estimation_svd.hpp]. */
int wm_umeyama_from_stats(const double stats[WM_STATS_LEN], double Tk_out[16]);
int wm_gn6_from_stats(const double stats[WM_STATS_LEN], double Tk_out[16]);

/* ------------------------------------------------------------------ GICP */
typedef struct {
    int corr_rand;        /* GICPMatcherParams::corr_rand, gicp.hpp:34 -> gicp.cpp:31 */
    int max_iter;         /* GICPMatcherParams::max_iter,  gicp.hpp:35 -> gicp.cpp:32 */
    double r_eps;         /* GICPMatcherParams::r_eps,     gicp.hpp:36 -> gicp.cpp:33 */
    double t_eps;         /* PCL default 5e-4 (libwave never sets it) */
    double max_corr;      /* PCL-GICP default 5 m (libwave never sets it) */
    double gicp_epsilon;  /* PCL default 1e-3 */
    int max_inner;        /* PCL default 20 BFGS iterations per outer iteration */
    int force_iterations; /* >0: exactly this many outer iterations (bench) */
    int objective;        /* how estimateRigidTransformationBFGS's objective is evaluated: WM_GICP_OBJECTIVE_* below */
    int reserved;
} wm_gicp_params;
/* WM_GICP_OBJECTIVE_PCL_SUMS (0, the default -- what the reference runs, wave_matching/src/gicp.cpp:58): PCL's per-pair
 * float path (OptimizationFunctorWithIndices::fdf summed pair by pair at every trial point), bit for bit the oracle's
 * default mode (oracle/gicp.c, objective mode 0).
 * WM_GICP_OBJECTIVE_STATISTICS (1, an explicit opt-in: NOT PCL's arithmetic): between two correspondence searches the
 * pairs and their Mahalanobis matrices are fixed and the residual is affine in the transform's entries, so the objective PCL sums pair by pair at
 * every trial point of the line search (OptimizationFunctorWithIndices::fdf, ~170 passes over the pairs per
 * registration) is formed ONCE per outer iteration as 74 sufficient statistics around the pairing transform; every
 * evaluation is then scalar work (libwave_amd/csrc/wm_gicp_quad.hpp).  The statistics' base point is PCL's float
 * residual; away from it the per-point float rounding of PCL's transform (a relative ~4e-7 of f) is absent.  PCL's
 * BFGS stops at a gradient tolerance of 1e-2 wherever its line search lands, so registrations of noisy pairs end
 * 1e-5 .. 1e-3 m apart between the two objectives -- the spread PCL's own result has against its summation order --
 * and pairs that register sharply (the reference's test cases) within 1e-4 m / 1e-5 rad; neither is systematically
 * closer to ground truth (tests/test_gicp_quad_gpu.py, tests/test_oracle_cpu.py).  That spread is ABOVE north_star's
 * 1e-4 m on noisy pairs, which is why this form is not the default.  Held bit for bit to the oracle's restatement of the
 * builder's reformulation (oracle/gicp.c, objective mode 1 -- a restatement check, not reference parity), on the
 * one-pair and the batched path.  The numbers equal the oracle's objective modes. */
#define WM_GICP_OBJECTIVE_PCL_SUMS 0
#define WM_GICP_OBJECTIVE_STATISTICS 1

typedef struct {
    int converged, iterations, n_corr, inner_total, evaluations;
    double f_final;
    float fdf_kernel_ms; /* summed device time of the objective/gradient kernel */
    int served_evaluations; /* of `evaluations`: answered by the resident evaluator (no kernel launch each) */
} wm_gicp_stats;

void wm_gicp_default_params(wm_gicp_params *p);
/* pcl::GeneralizedIterativeClosestPoint::align + hasConverged + getFinalTransformation
 * (wave_matching/src/gicp.cpp:58-60) on the clouds given by wm_set_source/wm_set_target.
 * Per-point covariances (computeCovariances, k = corr_rand) are computed on device and
 * cached per cloud. */
int wm_gicp_align(wm_ctx *ctx, const wm_gicp_params *p, double T_out[16], wm_gicp_stats *stats);
/* GICPMatcher::setRef + setTarget + match in one call (gicp.cpp:37-64): both clouds are
 * voxel-filtered on device when res > 0. */
int wm_gicp_match(wm_ctx *ctx, const void *ref, size_t n_ref, const void *target, size_t n_target,
                  size_t stride_bytes, int mem, const wm_gicp_params *p, float res, double T_out[16],
                  wm_gicp_stats *stats);
/* GICPMatcher::setRef / setTarget with res > 0 (wave_matching/src/gicp.cpp:38-45, 48-55): VoxelGrid
 * the cloud on the device and make the FILTERED copy the registration's source / target -- at the
 * time of the call (a snapshot, as the reference's filtered copy is). */
int wm_set_source_filtered(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, float leaf);
int wm_set_target_filtered(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, float leaf);
/* GICPMatcher::setRef + setTarget + match (wave_matching/src/gicp.cpp:37-64) for MANY pairs in one launch --
 * what a wave::MultiMatcher<GICPMatcher> has waiting in its queue (multi_matcher.hpp:29-34): one registration per
 * compute unit, the whole of align inside the kernel (grids, covariances, the outer loop with its 1-NN search,
 * Mahalanobis matrices and the BFGS minimisation -- the optimiser's code runs on the device here).
 *   res > 0: every cloud of the batch is voxel-filtered first (one pass of device-wide kernels), as
 *            setRef / setTarget do; res <= 0: the clouds as given, at most WM_GICP_BATCH_MAX_POINTS points each
 *            (beyond: WM_ERR_ARG).  A pair whose FILTERED cloud is larger is registered by wm_gicp_match.
 * Per item k: status[k] as wm_gicp_match would return it (WM_OK / WM_NOT_CONVERGED / WM_TOO_FEW_CORRESPONDENCES;
 * WM_ERR_STATE for an empty cloud), T_out + 16 k written when WM_OK, stats[k] (may be NULL).
 * Same neighbours, covariances, objective terms and (double-double) sums as wm_gicp_align, and the float
 * sinf / cosf / atan2f / asinf PCL's transform goes through are glibc's algorithms restated (wm_bfgs.hpp), so on
 * every pair tested the transform, objective value and iteration / evaluation counts EQUAL the one-pair path's and
 * the oracle's -- which is what tests/test_gicp_batch_gpu.py asserts (np.array_equal).  What is GUARANTEED is
 * 1e-6 m / 1e-6 rad: the double sin / cos of the gradient's rotation part are the device library's, and a
 * last-bit difference there can, after hundreds of evaluations of a registration that does not converge, take a
 * line-search branch the other way.
 * kernel_ms (may be NULL): device time of the launch. */
#define WM_GICP_BATCH_MAX_POINTS 100000
int wm_gicp_batch_match(wm_ctx *ctx, const wm_batch_item *items, int n_items, size_t stride_bytes, int mem,
                        const wm_gicp_params *p, float res, double *T_out, wm_gicp_stats *stats, int *status,
                        float *kernel_ms);
/* OptimizationFunctorWithIndices::fdf once: pairs + Mahalanobis matrices formed with
 * T_pair as one outer iteration does, then f and gradient at x = (t, roll, pitch, yaw). */
int wm_gicp_eval(wm_ctx *ctx, const wm_gicp_params *p, const double T_pair[16], const double x[6],
                 double *f, double g[6], int *n_pairs);
/* computeCovariances of both clouds (9 doubles per point, caller order); either output
 * may be NULL (kernel-level parity).  k: 1 ... 32; WM_NOT_CONVERGED when a cloud has fewer than k finite
 * points (PCL refuses to align then), nothing written. */
int wm_gicp_covariances(wm_ctx *ctx, int k, double eps, double *cov_source, double *cov_target);

/* ------------------------------------------------------------------- NDT */
typedef struct {
    double res;           /* NDTMatcherParams::res,       ndt.hpp:40 -> ndt.cpp:32 setResolution */
    double step_size;     /* NDTMatcherParams::step_size, ndt.hpp:37 -> ndt.cpp:31 setStepSize  */
    double t_eps;         /* NDTMatcherParams::t_eps,     ndt.hpp:39 -> ndt.cpp:30              */
    int max_iter;         /* NDTMatcherParams::max_iter,  ndt.hpp:38 -> ndt.cpp:33              */
    double outlier_ratio; /* PCL default 0.55 (not set by libwave) */
    int skip_line_search; /* 1: PCL 1.8.x behaviour (More-Thuente loop never runs) */
    int pcl_d1_sign;      /* 1: PCL's h_ang_d1[2] = +sy; 0: the true derivative -sy */
    int force_iterations; /* >0: exactly this many Newton iterations (bench) */
} wm_ndt_params;

typedef struct {
    int converged, iterations, n_voxels, evaluations;
    double score;          /* trans_probability_: score / number of source points */
    float deriv_kernel_ms; /* summed device time of the derivative kernel; 0 unless WM_NDT_PROFILE=1 */
    int model_builds;      /* voxel models this context has built so far (an unchanged target keeps its
                              model across align calls, as PCL's setInputTarget does) */
} wm_ndt_stats;

void wm_ndt_default_params(wm_ndt_params *p);
/* pcl::NormalDistributionsTransform::align + hasConverged + getFinalTransformation
 * (wave_matching/src/ndt.cpp:59-61) on the clouds given by wm_set_source /
 * wm_set_target; the voxel statistics of setInputTarget (ndt.cpp:55) are (re)built on
 * device when the target or `res` changed. */
int wm_ndt_align(wm_ctx *ctx, const wm_ndt_params *p, double T_out[16], wm_ndt_stats *stats);
/* pcl::NormalDistributionsTransform::setInputTarget builds the voxel grid when it is called
 * (wave_matching/src/ndt.cpp:55): the model of the current target at resolution `res`, now; later
 * wm_ndt_align calls with the same target and res reuse it. */
int wm_ndt_build_model(wm_ctx *ctx, double res);
/* NDTMatcher::setRef + setTarget + match (wave_matching/src/ndt.cpp:48-65) for MANY pairs in one launch -- what a
 * wave::MultiMatcher<NDTMatcher> has waiting in its queue (multi_matcher.hpp:29-34): one registration per compute unit,
 * the target's voxel model (pcl::VoxelGridCovariance), the Newton steps and the More-Thuente line search all inside the
 * kernel.  Clouds of at most WM_NDT_BATCH_MAX_POINTS points (beyond: WM_ERR_ARG); a pair whose voxel lattice does not
 * fit the kernel's table (262 144 cells) is registered by wm_ndt_align.
 * Per item k: status[k] as wm_ndt_align would return it (WM_OK / WM_NOT_CONVERGED; WM_ERR_STATE for an empty cloud;
 * WM_ERR_ARG for a target spanning more than 2^20 voxels along an axis -- e.g. one far-away garbage return),
 * T_out + 16 k written when WM_OK, stats[k] (may be NULL).  Same voxel membership, radius tests and terms as
 * wm_ndt_align; a voxel's sums are formed in double-double instead of in point order and exp / log / sin / cos are the
 * device library's: results agree with the one-pair path to ~1e-9, not bit for bit. */
#define WM_NDT_BATCH_MAX_POINTS 200000
int wm_ndt_batch_match(wm_ctx *ctx, const wm_batch_item *items, int n_items, size_t stride_bytes, int mem,
                       const wm_ndt_params *p, double *T_out, wm_ndt_stats *stats, int *status, float *kernel_ms);
/* computeDerivatives at pose (tx,ty,tz,rx,ry,rz): score, gradient(6), Hessian(36) */
int wm_ndt_derivatives(wm_ctx *ctx, const wm_ndt_params *p, const double pose[6], double *score,
                       double grad[6], double hess[36], int *n_voxels);

/* ---------------------------------------------- sharded registration (multi-GPU)
 * One registration spread over the GPUs of a node, one process (rank) per GPU:
 * every rank holds the full source cloud and the target points of one x-slab
 * [x_lo - max_corr, x_hi + max_corr] (wm_set_target of that subset), handles the
 * source points whose TRANSFORMED x falls into [x_lo, x_hi) (so each source point
 * is handled by exactly one rank and its true neighbour within max_corr is in that
 * rank's subset), and the WM_STATS_LEN-double statistics block is summed over ranks
 * (RCCL all-reduce over xGMI) once per iteration; every rank then applies the same
 * solve, so the transform never needs broadcasting.
 *   wm_icp_shard_begin        reset the iteration state (like the start of align())
 *   wm_icp_shard_local_stats  enqueue search + reduction; writes this rank's partial
 *                             statistics to stats_dev (WM_STATS_LEN doubles in HBM)
 *   <caller all-reduces stats_dev (sum) on a stream ordered after the ctx stream>
 *   wm_icp_shard_apply        enqueue the solve + stopping rules from stats_dev
 *   wm_icp_shard_poll         sync; report done / transform / statistics
 * All enqueue calls are asynchronous on the context's stream (wm_ctx_set_stream).
 * A rank need not hold the full source cloud: any superset of the points that can fall
 * into its slab will do (e.g. those within a band around the slab).  To keep that exact,
 * pass expect_owned_total = the number of (finite) source points of the whole cloud:
 * stats[WM_STATS_LEN-1] carries the number of points each rank handled, and every
 * iteration in which the all-reduced count differs is tallied in
 * wm_icp_stats.owned_violations -- the caller then redoes the registration with wider
 * bands / full clouds.  0 disables the check. */
int wm_icp_shard_begin(wm_ctx *ctx, const wm_icp_params *p, double x_lo, double x_hi,
                       size_t expect_owned_total);
int wm_icp_shard_local_stats(wm_ctx *ctx, void *stats_dev);
int wm_icp_shard_apply(wm_ctx *ctx, const void *stats_dev);
int wm_icp_shard_poll(wm_ctx *ctx, int *done, double T_out[16], wm_icp_stats *stats);

/* Sharded NDT ("replicate the target, shard ref by index range"; no reference
 * counterpart -- PCL's NDT is single-threaded).  Every rank sets the SAME two clouds and builds
 * the same voxel model (cheap: < 0.5 ms at 2M points); the Morton-ordered source is dealt out
 * to the ranks in chunks of 4096 points, round-robin (every rank works on the whole scene at
 * 1/world density: equal work), rank r evaluates its chunks in every derivative pass, and the
 * sums of that pass -- n = 28 (score, gradient, upper triangle of the Hessian) or n = 7 (score,
 * gradient: the line search's passes) -- are summed over the ranks by `reduce` before the
 * Newton / More-Thuente logic sees them.  `reduce` must leave bit-identical
 * values on every rank (an RCCL / gloo all-reduce does): all ranks then take the same decisions
 * and return the same transform, with no broadcast.  It is called on the thread that called
 * wm_ndt_align, with a host array; return 0 on success (anything else aborts the registration
 * with WM_ERR_STATE).  world = 1 or reduce = NULL restores the single-GPU behaviour. */
typedef int (*wm_allreduce_fn)(double *vals, int n, void *user);
int wm_ndt_set_shard(wm_ctx *ctx, int rank, int world, wm_allreduce_fn reduce, void *user);

/* ------------------------------------------ sharded registration, driven from C (RCCL inside)
 * A wm_comm is one rank's handle on a group of `world` ranks, one GPU each (librccl is linked into this
 * library).  The ICP loop's exchange step -- 34 doubles per rank and iteration -- goes through MAILBOXES where
 * they can be set up: fine-grained device memory of every rank, mapped into its peers (IPC handles all-gathered
 * over the communicator between processes, peer access inside one), into which the solve kernel of every rank
 * stores its block over xGMI and out of which it adds all blocks in rank order (csrc/wm_xchg.hpp: no launch
 * between a rank's sums and its solve).  A probe exchange at creation and an all-reduced verdict decide, alike
 * on every rank, whether they are used; otherwise, and with WM_COMM_P2P=0, the step is an RCCL all-reduce on the
 * calling context's stream.  A peer whose block does not arrive within WM_COMM_P2P_TIMEOUT_MS (default 5000)
 * fails the registration with WM_ERR_RCCL instead of hanging -- and that rank's communicator then goes back to the
 * collective exchange for good (wm_multi_* run the failed registration once more by themselves; bench.py --gpus N
 * rebuilds its communicators without mailboxes if its first registration fails on any rank).
 * wm_icp_stats.exchange_in_kernel says which exchange ran.
 * No reference counterpart: libwave's only parallelism is one matcher per thread
 * (wave_matching/include/wave/matching/multi_matcher.hpp:32).
 *   wm_comm_get_unique_id + wm_comm_init_rank   one rank per process (or thread): rank 0 creates the
 *        128-byte id, the launcher hands it to every rank (bench.py: torch.distributed broadcast;
 *        MPI_Bcast; a file), every rank calls init_rank on its device.   = ncclCommInitRank
 *   wm_comm_init_all     all ranks in one process, `devices[r]` for rank r.  = ncclCommInitAll
 *   wm_comm_init_local   test stand-in: `n` ranks on ONE device whose all-reduce is a host-side sum
 *        in rank order at a barrier (each rank must run on its own thread).  WM_COMM_P2P_LOCAL=1 gives these
 *        ranks mailboxes too (tests of the protocol; on one GPU a rank's first-call allocations wait for the
 *        other rank's polling kernel, so contexts must have registered once before). */
typedef struct wm_comm wm_comm;
#define WM_COMM_ID_BYTES 128
int wm_comm_get_unique_id(void *id_out /* WM_COMM_ID_BYTES */);
int wm_comm_init_rank(wm_comm **out, int device, const void *id, int rank, int world);
int wm_comm_init_all(wm_comm **comms /* [n] */, const int *devices, int n);
int wm_comm_init_local(wm_comm **comms /* [n] */, int n, int device);
void wm_comm_destroy(wm_comm *comm);
/* us per exchange of the loop's block (the mailbox exchange in a kernel of its own, or ncclAllReduce), `reps` back
 * to back on the context's stream (collective) */
int wm_comm_allreduce_probe(wm_ctx *ctx, wm_comm *comm, int reps, double *us_out);
int wm_comm_rank(const wm_comm *comm);
int wm_comm_world(const wm_comm *comm);
/* 1 while the group's sharded ICP loop exchanges through the ranks' mailboxes, 0 once it uses ncclAllReduce (never set
 * up, WM_COMM_P2P=0, or dropped after an exchange that failed -- on EVERY rank alike: the loop's commit round makes the
 * ranks agree).  wm_comm_set_exchange_timeout_ms: how long a solve kernel waits for a peer's block (default 5000 ms;
 * 0 = a block that is not there at once counts as never coming: tests). */
int wm_comm_mailboxes(const wm_comm *comm);
int wm_comm_set_exchange_timeout_ms(wm_comm *comm, int ms);

/* pcl::IterativeClosestPoint::align (wave_matching/src/icp.cpp:126-129) as ONE registration over
 * all ranks of `comm`.  Collective: every rank calls it with the same two (full) clouds and
 * parameters, on its own context (`mem` = where the clouds live for THIS rank).  Inside the call:
 * equal-count x-slabs of the target from a histogram of a fixed sub-sample of 16 384 points (identical on
 * all ranks, no communication), this rank's slab + max_corr halo of the target and its band of the source
 * selected out of the clouds as the caller laid them out (one stable compaction of both), the index over
 * them, then per iteration search + local sums -> exchange of 34 doubles (the ranks' mailboxes inside the
 * solve kernel, or ncclAllReduce: see wm_comm above) -> solve, all enqueued on the context's stream.  A peer
 * whose block does not arrive in time fails this rank's call with WM_ERR_RCCL.  Host clouds: with an RCCL communicator rank 0 uploads, the others receive
 * over xGMI (ncclBroadcast).  Every rank returns the same transform and status; `stats` carries the
 * rank's per-phase budget.  A rank that fails with a HIP / RCCL error aborts the communicator (its
 * peers' pending collectives fail instead of waiting for ever); the communicator is finished then.
 * comm == NULL or a world of 1 is plain wm_set_source + wm_set_target + wm_icp_align. */
int wm_icp_align_sharded(wm_ctx *ctx, wm_comm *comm, const void *ref, size_t n_ref, const void *target,
                         size_t n_target, size_t stride_bytes, int mem, const wm_icp_params *p,
                         double T_out[16], wm_icp_stats *stats);
/* ICPMatcher::match() (wave_matching/src/icp.cpp:75-133) over the ranks of `comm`, voxel-filtered
 * branches included -- the reference's DEFAULT parameters (res 0.1, three coarser scales,
 * icp.hpp:54,59): every rank filters both clouds itself (deterministic: all hold the same filtered
 * clouds) and the align of every scale is sharded.  res <= 0: wm_icp_align_sharded. */
int wm_icp_match_sharded(wm_ctx *ctx, wm_comm *comm, const void *ref, size_t n_ref, const void *target,
                         size_t n_target, size_t stride_bytes, int mem, const wm_icp_params *p, float res,
                         int multiscale_steps, double T_out[16], wm_icp_stats *stats);
/* wm_icp_info after a sharded registration (ICPMatcher::estimateInfo, icp.cpp:135-142).  Collective:
 * every rank adds up the pairs of the queries it owned, the 16 / 1 / 42 sums are exchanged over `comm`,
 * every rank finishes the same 6x6.  (wm_icp_info itself refuses after a sharded align: one rank's
 * pairs alone say nothing.) */
int wm_icp_info_sharded(wm_ctx *ctx, wm_comm *comm, int method, const double T_result[16], double lin_covar,
                        double ang_covar, double max_corr, double info_out[36], int *degenerate);

/* Sharded NDT with the exchange on the device: like wm_ndt_set_shard, but the sums of every
 * derivative pass are all-reduced in HBM over `comm` (RCCL) before the host fetches them -- no
 * callback, no host bounce.  comm == NULL switches sharding off. */
int wm_ndt_set_comm(wm_ctx *ctx, wm_comm *comm);

/* --------------------------------------------------------- ground segmentation */
/* wave::GroundSegmentationParams (wave_matching/include/wave/matching/ground_segmentation_params.hpp:10-37):
 * the same fields, types and defaults (wm_ground_default_params). */
typedef struct {
    double rmax;            /* :11  points at this radius or beyond get no label */
    int max_bin_points;     /* :12  parsed, never used (as in the reference) */
    int num_seed_points;    /* :13  seeds per sector; < 0: every eligible signal point */
    float p_l;              /* :16  GP length scale (> 0) */
    float p_sf;             /* :18  GP signal scale (> 0) */
    float p_sn;             /* :19  GP noise (> 0) */
    float p_tmodel;         /* :20  inlier: predicted variance below this ... */
    float p_tdata;          /* :23  ... and normalised residual below this */
    float p_tg;             /* :25  ground: within this of the model height */
    double robot_height;    /* :28  overhanging: above this over the model */
    double max_seed_range;  /* :31 */
    double max_seed_height; /* :32 */
    int num_bins_a;         /* :34  angular sectors (> 0) */
    int num_bins_l;         /* :35  linear bins per sector (> 0) */
} wm_ground_params;
void wm_ground_default_params(wm_ground_params *p);

/* per-point labels (labels_out) and the lists of the keep mask */
enum { WM_GROUND_NONE = 0, WM_GROUND_GROUND = 1, WM_GROUND_OBSTACLE = 2, WM_GROUND_OVERHANGING = 3 };
enum { WM_KEEP_GROUND = 1, WM_KEEP_OBSTACLE = 2, WM_KEEP_OVERHANGING = 4 };

typedef struct {
    size_t n_ground, n_obstacle, n_overhanging;  /* the three lists' sizes, whatever the keep mask */
    size_t n_in_range;                           /* points with radius < rmax */
    int n_signal_cells;                          /* cells of more than 5 points (impl :123) */
    int n_model_cells;                           /* cells in a sector's final ground model (seeds included) */
    int n_sufficient_sectors;                    /* sectors with at least 2 seeds (impl :182) */
    int passes_total, passes_max;                /* INSAC passes, summed and the largest of a sector */
} wm_ground_stats;

/* GroundSegmentation<PointT>::applyFilter (wave_matching/include/wave/matching/impl/ground_segmentation.hpp:358-381):
 * genPolarBinGrid (:36-84) and sectorINSAC per sector (:108-355) on the device.  The indices of the kept lists --
 * ground, then obstacle, then overhanging, each ordered by sector, within a sector model cells (model order) then
 * the remaining cells (ascending height), within a cell ascending index -- go to indices_out (`out_mem` says where
 * it lives, as labels_out, whose n entries are WM_GROUND_* per input point; NULL: not wanted).  *n_out = the kept
 * points; more than `cap`: WM_ERR_ARG (the first `cap` are written).  Every call classifies its input afresh.
 * Parameters that would make the reference index out of bounds or divide into NaN are WM_ERR_ARG: num_bins_a or
 * num_bins_l <= 0, p_l, p_sf or p_sn <= 0, any non-finite value.  num_bins_a * num_bins_l above 2^24, or device
 * memory short of what the sectors' GP factors need (m^2 + m (m + 1) / 2 doubles for a sector of m signal cells):
 * WM_ERR_NOMEM.  The workspace is the context's own (grown on demand -- a call whose factors outgrow it runs its
 * sector stage twice -- and freed by wm_ctx_destroy); a context's registration state (clouds, grid, models) is not
 * touched. */
int wm_ground_segment(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                      const wm_ground_params *params, int keep_mask, int32_t *indices_out, size_t cap, int out_mem,
                      size_t *n_out, uint8_t *labels_out /* NULL ok */, wm_ground_stats *stats /* NULL ok */);

/* One scan of a batch: n records of `stride_bytes`, x y z first, in the memory the call's `mem` names. */
typedef struct {
    const void *pts;
    size_t n;
} wm_ground_scan;
/* What one batch may hold.  A point's sort key is scan * (cells + 1) + cell (cells = num_bins_a * num_bins_l, the
 * extra key per scan: out of range) in 32 bits, and a point's place in the batch a 31-bit index (as wm_ground_segment's
 * n).  Nothing else bounds the number of scans but the device memory their cells take (WM_ERR_NOMEM / WM_ERR_HIP). */
#define WM_GROUND_BATCH_MAX_KEYS 0xFFFFFFFFull  /* n_scans * (cells + 1) at most */
#define WM_GROUND_BATCH_MAX_POINTS 0x7FFFFFF0ull /* the scans' points in all, at most */

/* GroundSegmentation<PointT>::applyFilter (wave_matching/include/wave/matching/impl/ground_segmentation.hpp:358-381,
 * which the reference calls once per scan) for `n_scans` scans in ONE sequence of launches and one wait for the
 * results (a second when the factor workspace has to grow): every scan's slice of indices_out (indices local to the
 * scan), its slice of labels_out (the scans' n entries one after the other) and stats[k] are EQUAL to what
 * wm_ground_segment gives for that scan alone with the same `params` and `keep_mask` -- one of each per batch.
 * offsets_out (host, n_scans + 1 entries): scan k's kept points are [offsets_out[k], offsets_out[k + 1]) of
 * indices_out and of points_out.  points_out (NULL: not wanted): per kept index the input point's x, y, z bit for bit
 * in records of `out_stride` bytes (>= 12, a multiple of 4; bytes beyond 12 are zero) -- in device memory a cloud
 * wm_icp_batch_match(mem = WM_MEM_DEVICE) takes as it is.  `out_mem` says where indices_out, points_out and
 * labels_out live.  Empty scans and scans without a finite point are legal and give empty slices; n_scans == 0 is
 * WM_OK with offsets_out[0] = 0.  More kept points than `cap`: WM_ERR_ARG with the offsets valid (the first `cap`
 * indices and points are written).  Argument errors (a null context, table or offsets, a bad stride, mem or keep
 * mask, parameters wm_ground_segment refuses, a batch beyond the two limits above) are found before a device is
 * touched.  kernel_ms (NULL ok): device time between the upload and the fetch of the counts.  The workspace is the
 * one wm_ground_segment uses; the context's registration state is not touched. */
int wm_ground_segment_batch(wm_ctx *ctx, const wm_ground_scan *scans, int n_scans, size_t stride_bytes, int mem,
                            const wm_ground_params *params, int keep_mask, int32_t *indices_out, size_t cap,
                            void *points_out /* NULL ok */, size_t out_stride, int out_mem, size_t *offsets_out,
                            uint8_t *labels_out /* NULL ok */, wm_ground_stats *stats /* NULL ok */,
                            float *kernel_ms /* NULL ok */);

/* ------------------------------------------------------------- outlier removal */
/* pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval on the device.  The rules are restated from PCL 1.8
 * (PCL is not linked; tests/outlier_reference.py is the checker):
 *   both         squared distances are float32, d2 = (dx * dx + dy * dy) + dz * dz with every operation rounded and
 *                nothing fused; kept indices ascend; negative != 0 returns the outliers instead of the inliers.
 *   statistical  [PCL-upstream filters/impl/statistical_outlier_removal.hpp]  per finite point its mean_k + 1 nearest
 *                points of the cloud, ordered by (d2, index), itself included; the first entry (d2 = 0: the point or a
 *                duplicate) is skipped; s = the sum of sqrt((double) d2) over the other mean_k, in list order, in
 *                double; the point's mean distance = (float) (s / mean_k).  Over the n finite points, the distances
 *                widened to double: mean = sum d / n, var = (sum d^2 - (sum d)^2 / n) / (n - 1), stddev = sqrt(var),
 *                threshold = mean + stddev_mult * stddev.  Outlier iff (double) dist > threshold; a NaN threshold
 *                removes nothing.  Fewer than mean_k + 1 finite points: WM_NOT_CONVERGED, nothing written.
 *                mean_k is 1 ... 31 (the k-NN search keeps lists of 32): beyond it WM_ERR_ARG.
 *   radius       [PCL-upstream filters/impl/radius_outlier_removal.hpp, FLANN's RadiusResultSet]  r2 = (float)
 *                (radius * radius), the product formed in double; a point's count = the OTHER finite points with
 *                d2 < r2 (strict); inlier iff count >= min_neighbors (PCL's "k <= min_pts is an outlier" with the
 *                point itself in k).  radius finite and > 0, min_neighbors >= 0, else WM_ERR_ARG.
 *   deviation    a non-finite point is nobody's neighbour, enters no statistic, gets WM_OUTLIER_NONE and is returned
 *                with neither setting of `negative` (PCL keeps such a point, with distance 0): wm_set_source drops
 *                them the same way. */
enum { WM_OUTLIER_STATISTICAL = 0, WM_OUTLIER_RADIUS = 1 };
enum { WM_OUTLIER_NONE = 0, WM_OUTLIER_INLIER = 1, WM_OUTLIER_OUTLIER = 2 };
typedef struct {
    int method;          /* WM_OUTLIER_STATISTICAL or WM_OUTLIER_RADIUS */
    int mean_k;          /* statistical: neighbours per point, 1 ... 31 */
    double stddev_mult;  /* statistical: threshold = mean + stddev_mult * stddev */
    double radius;       /* radius: metres, finite and > 0 */
    int min_neighbors;   /* radius: inlier with at least this many other points inside */
    int negative;        /* != 0: return the outliers */
} wm_outlier_params;
typedef struct {
    size_t n_finite, n_inliers, n_outliers;
    double mean, stddev, threshold;  /* statistical; 0 in radius mode */
    float kernel_ms;                 /* device time from the cloud's packing to the kept list (the grid's two small
                                        fetches to the host included) */
} wm_outlier_stats;
void wm_outlier_default_params(wm_outlier_params *p);  /* PCL's: mean_k 1, stddev_mult 0, radius 0, min_neighbors 1 */

/* One filter pass over n records of `stride_bytes` (x y z first) in `mem`.  indices_out: the kept points' indices,
 * ascending; *n_out their number; more than `cap`: WM_ERR_ARG with the first `cap` written and *n_out the true count.
 * `out_mem` says where all four output arrays live.  labels_out (NULL ok): WM_OUTLIER_* per input point.
 * mean_dist_out (NULL ok, statistical): the mean distance per point, 0 for a non-finite one.  counts_out (NULL ok,
 * radius): the exact neighbour count per point, -1 for a non-finite one; without it a point's search stops once it
 * has seen min_neighbors.  Argument errors (a null context, params or n_out, a bad stride, mem or method, parameters
 * out of range) are found before a device is touched.  n == 0 or a cloud without a finite point: WM_OK, *n_out = 0.
 * The cloud's grid is built for the call; the workspace is the context's own (grown on demand, freed by
 * wm_ctx_destroy); a context's registration state (clouds, grids, cached covariances and normals, tuned cell sizes)
 * is not touched. */
int wm_outlier_filter(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                      const wm_outlier_params *p, int32_t *indices_out, size_t cap, int out_mem, size_t *n_out,
                      uint8_t *labels_out /* NULL ok */, float *mean_dist_out /* NULL ok, statistical */,
                      int32_t *counts_out /* NULL ok, radius; -1 for a non-finite point */,
                      wm_outlier_stats *stats /* NULL ok */);

/* A queue of scans in one device call: the same steps with a scan dimension, one `p`, one stride and one `mem` for
 * the batch (as wm_ground_segment_batch and wm_cluster_extract_batch), in a number of launches and host waits that
 * does not depend on n_scans.  For every scan k, status[k], the slice [offsets_out[k], offsets_out[k + 1]) of
 * indices_out (indices local to the scan, ascending), its slices of labels_out, mean_dist_out and counts_out (the
 * scans' n entries one after the other) and stats[k] (but kernel_ms, which is the batch's) EQUAL what
 * wm_outlier_filter returns for that scan alone with the same `p` -- the bits of mean, stddev and threshold included,
 * whatever the other scans of the batch are and whatever their order.  points_out (NULL: not wanted): per kept index
 * the input point's x y z, bit for bit, in records of out_stride bytes (>= 12, a multiple of 4; the bytes behind z are
 * zero) -- wm_ground_segment_batch's rules, and what wm_cluster_extract_batch(mem = WM_MEM_DEVICE) takes as it is.
 * out_mem says where indices_out, points_out, labels_out, mean_dist_out and counts_out live; offsets_out (n_scans + 1
 * entries), status and stats (n_scans entries) are host memory.
 * The call returns WM_OK when the batch ran.  A statistical scan with 0 < n_finite < mean_k + 1 has status[k] =
 * WM_NOT_CONVERGED, an empty slice of indices and stats[k] zero but n_finite; its slices of labels, distances and
 * counts hold 0 / WM_OUTLIER_NONE and carry no meaning; its points are not searched.  Empty scans and scans without a
 * finite point are WM_OK with empty slices (labels NONE, distance 0, count -1).  n_scans == 0, or no point in any
 * scan: WM_OK with no device touched and every offset 0.  More kept points than `cap`: WM_ERR_ARG with the offsets the
 * true ones (the first `cap` indices and points are written).  Argument errors, found before a device is touched:
 * wm_outlier_filter's, a null scans / offsets_out / status, a scan with a null pts and n > 0, a bad out_stride with
 * points_out, and a batch beyond the two limits below.  A batch of one scan is the single call.
 * Each scan has a lattice of its own; where the single call allows a scan 2^26 + 8 n cells, a batch allows scan k
 * 8 n_k + max(2^26 / n_scans, 4096): one 2^26 for the whole batch (wm_cluster_extract_batch's rule).  Coarser cells
 * change no output.  kernel_ms (NULL ok): device time from the upload to the kept list.  The workspace is the one of
 * wm_outlier_filter; the registration state and the ground and cluster workspaces are not touched. */
typedef struct { const void *pts; size_t n; } wm_outlier_scan;
#define WM_OUTLIER_BATCH_MAX_POINTS 0x7FFFFFF0ull /* the scans' points in all, at most */
#define WM_OUTLIER_BATCH_MAX_SCANS 0x1000000ull   /* n_scans at most */
int wm_outlier_filter_batch(wm_ctx *ctx, const wm_outlier_scan *scans, int n_scans, size_t stride_bytes, int mem,
                            const wm_outlier_params *p,
                            int32_t *indices_out, size_t cap,
                            void *points_out /* NULL ok */, size_t out_stride,
                            int out_mem, size_t *offsets_out /* host, n_scans + 1 entries */,
                            uint8_t *labels_out /* NULL ok */, float *mean_dist_out /* NULL ok, statistical */,
                            int32_t *counts_out /* NULL ok, radius */,
                            int *status /* host, n_scans entries */, wm_outlier_stats *stats /* NULL ok: n_scans entries */,
                            float *kernel_ms /* NULL ok */);

/* ------------------------------------------------------------- Euclidean cluster extraction */
/* pcl::EuclideanClusterExtraction on the device: the step between GroundSegmentation's obstacle points and a
 * registration.  [PCL-upstream: restated from PCL 1.8 segmentation/impl/extract_clusters.hpp; no PCL on the build
 * machine]  (tests/cluster_reference.py is the checker):
 *   edges        r2 = (float) (tolerance * tolerance), the product formed in double; two different finite points are
 *                joined iff d2 < r2 (strict, as FLANN's radius set under PCL's clustering), d2 = (dx * dx + dy * dy) +
 *                dz * dz in float with every operation rounded and nothing fused.  That form is symmetric in its two
 *                points: the relation is an undirected graph.
 *   clusters     PCL's region growing (extractEuclideanClusters) returns that graph's connected components, whatever
 *                the seed order.  A component is grown in full and kept iff max(min_cluster_size, 1) <= size <=
 *                max_cluster_size; max < min is legal and keeps nothing.
 *   order        clusters by size, largest first (EuclideanClusterExtraction::extract sorts them so); inside a cluster
 *                the indices ascend (PCL sorts them).  Cluster c is indices_out[offsets_out[c] .. offsets_out[c + 1]);
 *                labels_out[i] is c, WM_CLUSTER_REJECTED or WM_CLUSTER_NONE.
 *   deviations   PCL leaves the order of equal-sized clusters to std::sort: here equal sizes go by their smallest
 *                member index, ascending.  A non-finite point is nobody's neighbour and is in no cluster
 *                (WM_CLUSTER_NONE), exactly as in wm_outlier_filter.
 *   determinism  every output byte is a function of the input array alone; two calls give identical bytes. */
typedef struct {
    double tolerance;      /* setClusterTolerance: metres, finite and > 0 */
    int min_cluster_size;  /* setMinClusterSize, >= 0 (0 acts as 1); PCL's default 1 */
    int max_cluster_size;  /* setMaxClusterSize, >= 0; PCL's default INT_MAX */
} wm_cluster_params;
void wm_cluster_default_params(wm_cluster_params *p);   /* PCL's: 0, 1, INT_MAX (tolerance must then be set) */

enum { WM_CLUSTER_NONE = -1 /* non-finite point */, WM_CLUSTER_REJECTED = -2 /* its component is outside [min, max] */ };
typedef struct {
    size_t n_finite, n_components /* before the size rule */, n_clusters, n_clustered /* points in kept clusters */,
        largest /* points of the largest KEPT cluster, 0 without one */;
    float kernel_ms;   /* pack to the last output, as wm_outlier_stats.kernel_ms */
} wm_cluster_stats;

/* One extraction over n records of `stride_bytes` (x y z first) in `mem`.  *n_clusters and *n_out: the kept clusters
 * and their points.  More kept points than `cap`, or more clusters than `cap_clusters`: WM_ERR_ARG with *n_out and
 * *n_clusters the true counts, the first `cap` indices and the first cap_clusters + 1 offsets written, the offsets
 * clamped to `cap`.  `out_mem` says where the three output arrays live.  Argument errors are found before a device is
 * touched: a null ctx / p / n_out / n_clusters, a bad stride, mem or out_mem, n > 0x7FFFFFF0, a tolerance that is not
 * finite or <= 0, negative sizes, a null array with a non-zero capacity.  n == 0 or a cloud without a finite point:
 * WM_OK with zero clusters and offsets_out[0] = 0 (for n == 0 no device is touched, so offsets_out[0] is written only
 * where out_mem is WM_MEM_HOST).  The grid is built for the call; the workspace is the context's own (freed by
 * wm_ctx_destroy); the registration state and the outlier and ground workspaces are not touched. */
int wm_cluster_extract(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                       const wm_cluster_params *p,
                       int32_t *labels_out /* NULL ok: n entries */,
                       int32_t *indices_out, size_t cap,              /* the clusters' members, back to back */
                       uint32_t *offsets_out, size_t cap_clusters,    /* cap_clusters + 1 entries */
                       int out_mem, size_t *n_clusters, size_t *n_out, wm_cluster_stats *stats /* NULL ok */);

/* pcl::ConditionalEuclideanClustering with a normal and / or a scalar test on every edge: what keeps a parked car
 * apart from the wall it stands against, or a kerb from the road.  [PCL-upstream: restated from PCL 1.8
 * segmentation/impl/conditional_euclidean_clustering.hpp; no PCL on the build machine]
 * (tests/cluster_cond_reference.py is the checker):
 *   attributes   `attr` holds n records of attr_stride bytes (>= 16, a multiple of 4) in attr_mem, record i belonging to
 *                point i; each begins with four floats (a0, a1, a2, s).  That is what wm_estimate_normals writes
 *                (nx, ny, nz, curvature), so its device output goes in as it is; s is whatever the caller puts there,
 *                an intensity for one.
 *   edges        two different finite points i, j are joined iff ALL of
 *                  d2 < r2, exactly as in wm_cluster_extract;
 *                  with WM_CLUSTER_COND_NORMAL: fabsf(dot) >= cos_min, dot = (a0_i * a0_j + a1_i * a1_j) + a2_i * a2_j
 *                    in float with every operation rounded and nothing fused, cos_min = (float) cos(max_normal_angle)
 *                    with the cosine taken in double;
 *                  with WM_CLUSTER_COND_SCALAR: fabsf(s_i - s_j) <= (float) max_scalar_diff, the subtraction one float
 *                    operation.
 *                Both tests are symmetric in i and j bit for bit, so the relation is an undirected graph and PCL's
 *                region growing returns its connected components whatever the seed order.  A NaN anywhere makes its
 *                comparison false: a finite point with NaN attributes is a component of its own, and so is one with
 *                the (0, 0, 0, .) normal wm_estimate_normals gives a degenerate neighbourhood as long as cos_min > 0
 *                -- a cluster of one point, not WM_CLUSTER_NONE.  (float) cos(pi / 2) is 6.1e-17, not 0: exactly
 *                perpendicular normals are separate even at max_normal_angle = pi / 2.  Switching the test off is what
 *                `flags` is for.
 *   the rest     the size rule, the order of the clusters and of their members, the labels, the capacities and their
 *                WM_ERR_ARG rule, n == 0, a cloud without a finite point (its attributes do not matter: a non-finite
 *                point is WM_CLUSTER_NONE), the workspace and the determinism are wm_cluster_extract's, word for word.
 *   flags == 0   attr may be NULL; the call returns byte for byte what wm_cluster_extract returns, from the same
 *                kernels.
 *   deviations   from PCL's class: the condition is one of these fixed tests, not a caller's function (and so always
 *                symmetric); PCL returns the clusters in seed order, here they are ordered as wm_cluster_extract's;
 *                there is no getRemovedClusters (labels_out says WM_CLUSTER_REJECTED instead).
 * Argument errors, found before a device is touched: wm_cluster_extract's; a null c; flags outside 0 ... 3;
 * reserved != 0; flags != 0 with a null attr and n > 0; an attr_stride below 16 or no multiple of 4, or a bad attr_mem
 * (both whatever the flags); with WM_CLUSTER_COND_NORMAL an angle that is not finite or outside [0, pi / 2]; with
 * WM_CLUSTER_COND_SCALAR a difference that is not finite or negative. */
enum { WM_CLUSTER_COND_NORMAL = 1, WM_CLUSTER_COND_SCALAR = 2 };
typedef struct {
    int flags;                /* OR of WM_CLUSTER_COND_*; 0: no edge test */
    int reserved;             /* 0 */
    double max_normal_angle;  /* radians, 0 ... pi/2; read with WM_CLUSTER_COND_NORMAL */
    double max_scalar_diff;   /* finite, >= 0;    read with WM_CLUSTER_COND_SCALAR */
} wm_cluster_cond;            /* 24 bytes */
void wm_cluster_cond_default(wm_cluster_cond *c);   /* all zero */

int wm_cluster_extract_cond(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                            const void *attr, size_t attr_stride, int attr_mem,
                            const wm_cluster_params *p, const wm_cluster_cond *c,
                            /* from here on exactly wm_cluster_extract's outputs */
                            int32_t *labels_out, int32_t *indices_out, size_t cap,
                            uint32_t *offsets_out, size_t cap_clusters, int out_mem,
                            size_t *n_clusters, size_t *n_out, wm_cluster_stats *stats);

/* A queue of scans in one device call: the same kernels with a scan dimension, one `p`, one stride and one `mem` for
 * the batch (as wm_ground_segment_batch).  The clusters of the batch are numbered scan after scan: scan k's are
 * [cluster_first[k], cluster_first[k + 1]), cluster_first[n_scans] is their number in all, and cluster g is
 * indices_out[offsets_out[g] .. offsets_out[g + 1]) -- indices inside its scan.  labels_out: the scans' n entries one
 * after the other, a cluster's rank INSIDE its scan, WM_CLUSTER_REJECTED or WM_CLUSTER_NONE.  points_out: per entry
 * of indices_out the input point's x y z, bit for bit, in records of out_stride bytes (>= 12, a multiple of 4; the
 * bytes behind z are zero) -- wm_ground_segment_batch's rules, and what wm_icp_batch_match takes as it is.  out_mem
 * says where labels_out, indices_out, points_out and offsets_out live; cluster_first (n_scans + 1 entries), n_out (the
 * kept points of all scans) and stats (n_scans entries) are host memory; kernel_ms, here and in every stats[k], is
 * the batch's.
 * For every scan k its labels, its indices, its offsets less offsets_out[cluster_first[k]] and stats[k] (but
 * kernel_ms) EQUAL what wm_cluster_extract returns for that scan alone.  Empty scans and scans without a finite point
 * have empty slices; n_scans == 0, or no point in any scan: WM_OK and no device touched (offsets_out[0] = 0 is then
 * written only where out_mem is WM_MEM_HOST).  More kept points than `cap` or more clusters than `cap_clusters`:
 * WM_ERR_ARG with *n_out and cluster_first the true counts, the first `cap` indices and points and the first
 * cap_clusters + 1 offsets written, the offsets clamped to `cap`.  Argument errors, found before a device is touched:
 * wm_cluster_extract's, a null scans / cluster_first, a scan with a null pts and n > 0, a bad out_stride with
 * points_out, and a batch beyond the limits below.  A batch of one scan is the single call.
 * Each scan has a lattice of its own; where the single call allows a scan 2^26 + 8 n cells, a batch allows scan k
 * 8 n_k + max(2^26 / n_scans, 4096): one 2^26 for the whole batch.  Coarser cells change no output.
 * The workspace is the one of wm_cluster_extract. */
typedef struct { const void *pts; size_t n; } wm_cluster_scan;
#define WM_CLUSTER_BATCH_MAX_POINTS 0x7FFFFFF0ull /* the scans' points in all, at most */
#define WM_CLUSTER_BATCH_MAX_SCANS 0x1000000ull   /* n_scans at most */
/* the kept clusters are ordered by ONE 64-bit key (scan, size, smallest member index):
 * bits(n_scans - 1) + 2 * bits(the largest scan's n) <= WM_CLUSTER_BATCH_KEY_BITS, bits(v) = the binary digits of v
 * (4 096 scans of 2^20 points: 12 + 2 * 21) */
#define WM_CLUSTER_BATCH_KEY_BITS 64
int wm_cluster_extract_batch(wm_ctx *ctx, const wm_cluster_scan *scans, int n_scans, size_t stride_bytes, int mem,
                             const wm_cluster_params *p,
                             int32_t *labels_out /* NULL ok: the scans' n entries one after the other */,
                             int32_t *indices_out, size_t cap,
                             void *points_out /* NULL ok */, size_t out_stride,
                             uint32_t *offsets_out, size_t cap_clusters /* cap_clusters + 1 entries */,
                             int out_mem,
                             size_t *cluster_first /* host, n_scans + 1 entries */,
                             size_t *n_out, wm_cluster_stats *stats /* NULL ok: n_scans entries */,
                             float *kernel_ms /* NULL ok */);

/* ------------------------------------------------------------- plane segmentation (RANSAC) */
/* pcl::SACSegmentation with a plane model and SAC_RANSAC on the device: one cloud in, one plane and its inliers out.
 * [PCL-upstream: restated from PCL 1.8 sample_consensus/impl/ransac.hpp (RandomSampleConsensus::computeModel),
 * sample_consensus/impl/sac_model_plane.hpp (SampleConsensusModelPlane) and segmentation/impl/sac_segmentation.hpp
 * (SACSegmentation::segment); no PCL on the build machine]  (tests/sac_reference.py is the checker).  All float
 * arithmetic below is float32 with every operation rounded and nothing fused.
 *   stream       DEVIATION (PCL draws its samples from rand() / boost): entry j = 0, 1, 2, ... of the hypothesis stream
 *                is a function of (seed, j, n) alone.  sm64(z), the splitmix64 finaliser, mod 2^64: z ^= z >> 30;
 *                z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *                r(j, a, m) = ((sm64(seed + 0x9E3779B97F4A7C15 * (3 j + a + 1)) >> 32) * m) >> 32.
 *                i0 = r(j, 0, n);  t = r(j, 1, n - 1), i1 = t + (t >= i0);  t = r(j, 2, n - 2), t += (t >= min(i0, i1)),
 *                t += (t >= max(i0, i1)), i2 = t.  Three distinct indices by construction, no retry loop; n counts
 *                all records, as PCL's indices do.
 *   plane        [computeModelCoefficients; DEVIATION: its collinearity test is replaced]  u = p1 - p0, v = p2 - p0,
 *                c = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), s = (c.x c.x + c.y c.y) + c.z c.z.
 *                The entry is SKIPPED iff s is not finite or not > 0 (a non-finite sample, a collinear one, underflow,
 *                overflow).  Otherwise l = sqrt(s), (a, b, c) = c / l, d = -((a p0.x + b p0.y) + c p0.z).
 *   axis models  WM_SAC_PERPENDICULAR_PLANE / WM_SAC_PARALLEL_PLANE: ax = the axis normalised in double and rounded to
 *                float, cos_eps / sin_eps = cos / sin(eps_angle) in double, rounded to float; dot = |(a ax.x + b ax.y)
 *                + c ax.z|.  PERPENDICULAR (the plane is perpendicular to the axis: its normal along it) is valid iff
 *                dot >= cos_eps, PARALLEL iff dot < sin_eps.  DEVIATION: PCL goes through acos.  An axis-invalid
 *                entry is an iteration with count 0 (PCL: countWithinDistance returns 0): while nothing has been
 *                counted yet, that 0 sets k as in PCL (w = 0, so the loop goes on); DEVIATION: it can never become
 *                the best model.
 *   count        [countWithinDistance / selectWithinDistance]  dist = |((a x + b y) + c z) + d|; a point is an inlier
 *                iff dist < thr, thr = the smallest float not below distance_threshold -- exactly PCL's (double) dist <
 *                threshold.  A non-finite point is never an inlier (WM_SAC_NONE).
 *   loop         [computeModel, literally, its quirks included]
 *                    it = 0; skipped = 0; k = 1.0; best = -1; max_skip = 10 * max_iterations
 *                    while it < k and skipped < max_skip:
 *                        take the next entry;  if it is skipped: ++skipped; continue
 *                        if the entry is axis-valid and count > best:
 *                            best = count;  w = count / n;  q = clamp(1 - w^3, eps, 1 - eps)   (eps = DBL_EPSILON)
 *                            k = log(1 - probability) / log(q)
 *                        else if it is axis-invalid and best == -1:  k = that with w = 0
 *                        ++it;  if it > max_iterations: break
 *                so up to max_iterations + 1 entries are evaluated, and an equal count never replaces the best.
 *                Without a best: WM_NOT_CONVERGED, nothing written, *n_out = 0; n < 3 the same without a device.
 *   refit        [optimizeModelCoefficients]  iff optimize_coefficients and the model has >= 4 inliers: the plane of
 *                the inliers' covariance, the eigenvector of its smallest eigenvalue in double, its components
 *                rounded to float TOWARD ZERO (never longer than the unit vector), d = -normal . centroid with that
 *                float normal, rounded to nearest; then the inliers are selected again with the refined coefficients
 *                (SACSegmentation's "Refine inliers").  DEVIATIONS: PCL sums uncentred floats, unusable at UTM offsets -- here the six
 *                second-order and three first-order sums (PCL's nine accumulators) are formed in double RELATIVE TO
 *                THE WINNING SAMPLE'S p0 and added exactly, in any order (integer limbs); the eigenvector's sign,
 *                which PCL leaves open, is fixed to agree with the model's normal; a non-finite result keeps the model.
 *   output       the inliers' indices ascending.  Every output byte is a function of the input array and the
 *                parameters; two calls give identical bytes; the model and the counts do not depend on how the stream
 *                is cut into rounds (option "sac_round"). */
enum { WM_SAC_PLANE = 0, WM_SAC_PERPENDICULAR_PLANE = 1, WM_SAC_PARALLEL_PLANE = 2 };
typedef struct {
    int model;                  /* WM_SAC_* */
    double distance_threshold;  /* finite and > 0 (PCL's default 0 selects nothing: WM_ERR_ARG here) */
    int max_iterations;         /* >= 1; PCL's default 50 */
    double probability;         /* in (0, 1); PCL's default 0.99 */
    int optimize_coefficients;  /* PCL's default 1 */
    double axis[3], eps_angle;  /* the two axis models: axis non-zero, 0 < eps_angle <= pi/2, else WM_ERR_ARG */
    uint64_t seed;              /* extension: PCL has no setter; default 0 */
} wm_sac_params;
void wm_sac_default_params(wm_sac_params *p);   /* PCL's: plane, 0 (the threshold must then be set), 50, 0.99, 1 */

enum { WM_SAC_NONE = 0 /* non-finite */, WM_SAC_INLIER = 1, WM_SAC_OUTLIER = 2 };
typedef struct {
    size_t n_finite, n_inliers_model /* the winning hypothesis' count */, n_inliers /* returned */;
    int iterations, skipped, rounds /* device rounds of the stream */, refined /* the refit replaced the model */;
    long long hypotheses /* stream entries consumed */, best_hypothesis /* its stream index, -1: none */;
    float model_coefficients[4]; /* the winning hypothesis before the refit */
    float kernel_ms;             /* pack to the last output */
} wm_sac_stats;

/* One segmentation over n records of `stride_bytes` (x y z first) in `mem`.  coefficients_out (host): a b c d of the
 * returned plane.  indices_out (cap entries) and labels_out (n bytes, WM_SAC_*) live in `out_mem`.  More inliers than
 * `cap`: WM_ERR_ARG with the first `cap` written and *n_out the true count.  Argument errors are found before a device
 * is touched: a null ctx / p / coefficients_out / n_out, a bad stride, mem or out_mem, n > 0x7FFFFFF0, a null pts with
 * n > 0, a null indices_out with cap > 0, an unknown model, and the parameter ranges above.  The workspace is the
 * context's own (freed by wm_ctx_destroy); the registration state and the ground, outlier and cluster workspaces are
 * not touched. */
int wm_sac_segment(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, const wm_sac_params *p,
                   float coefficients_out[4] /* host */, int32_t *indices_out, size_t cap, int out_mem,
                   size_t *n_out, uint8_t *labels_out /* NULL ok */, wm_sac_stats *stats /* NULL ok */);

/* A queue of scans in one device call: the same steps with a scan dimension, one `p` (its seed included), one stride
 * and one `mem` for the batch (as wm_outlier_filter_batch and wm_cluster_extract_batch), in a number of launches and
 * host waits that does not depend on n_scans: the front, one round trip per round of the longest-living scan, one for
 * the refit and one for the offsets.  For every scan k, status[k], coefficients_out + 4 k, the slice [offsets_out[k],
 * offsets_out[k + 1]) of indices_out (indices local to the scan, ascending), its slice of labels_out (the scans' n
 * entries one after the other) and stats[k] (but kernel_ms, which is the batch's) EQUAL what wm_sac_segment returns for
 * that scan alone with the same `p` -- rounds, hypotheses, best_hypothesis, the bits of model_coefficients, refined
 * and the bits of the refitted coefficients included, whatever the other scans of the batch are and whatever their
 * order: the hypothesis stream of scan k is a function of (seed, j, n_k), as in the single call.
 * negative != 0: indices_out / points_out hold the finite points that are NOT inliers of the returned plane, ascending
 * -- the points the single call labels WM_SAC_OUTLIER.  Labels, coefficients and stats are the same with either
 * setting; stats[k].n_inliers stays the inliers' number.
 * points_out (NULL: not wanted): per entry of indices_out the input point's x y z, bit for bit, in records of
 * out_stride bytes (>= 12, a multiple of 4; the bytes behind z are zero) -- wm_ground_segment_batch's rules, and what
 * wm_cluster_extract_batch(mem = WM_MEM_DEVICE) takes as it is.  out_mem says where indices_out, points_out and
 * labels_out live; coefficients_out (4 floats per scan), offsets_out (n_scans + 1 entries), status and stats (n_scans
 * entries) are host memory.
 * The call returns WM_OK when the batch ran.  A scan without a model (n < 3, or the all-skipped and all-refused exits)
 * has status[k] = WM_NOT_CONVERGED and an empty slice with either setting of `negative`; its coefficients are not
 * written, stats[k] is as the single call leaves it, its slice of labels holds WM_SAC_NONE and carries no meaning.  A
 * scan with n < 3 costs no device work.  n_scans == 0, or no scan with n >= 3: WM_OK with no device touched, every
 * offset 0 and every status WM_NOT_CONVERGED (labels_out is then written only where out_mem is WM_MEM_HOST).  More
 * entries than `cap`: WM_ERR_ARG with the offsets the true ones (the first `cap` indices and points are written).
 * Argument errors, found before a device is touched: wm_sac_segment's, a null scans / offsets_out / status /
 * coefficients_out (with n_scans == 0 too), a scan with a null pts and n > 0, a bad out_stride with points_out, a null
 * indices_out with cap > 0, and a batch beyond the two limits below.  A batch of one scan is the single call.
 * kernel_ms (NULL ok): device time from the upload to the offsets.  The workspace is the one of wm_sac_segment; the
 * registration state and the ground, outlier and cluster workspaces are not touched. */
typedef struct { const void *pts; size_t n; } wm_sac_scan;
#define WM_SAC_BATCH_MAX_POINTS 0x7FFFFFF0ull /* the scans' points in all, at most */
#define WM_SAC_BATCH_MAX_SCANS 0x1000000ull   /* n_scans at most */
int wm_sac_segment_batch(wm_ctx *ctx, const wm_sac_scan *scans, int n_scans, size_t stride_bytes, int mem,
                         const wm_sac_params *p, int negative,
                         float *coefficients_out /* host, 4 per scan */,
                         int32_t *indices_out, size_t cap,
                         void *points_out /* NULL ok */, size_t out_stride, int out_mem,
                         size_t *offsets_out /* host, n_scans + 1 entries */,
                         uint8_t *labels_out /* NULL ok: the scans' n entries one after the other */,
                         int *status /* host, n_scans entries */, wm_sac_stats *stats /* NULL ok: n_scans entries */,
                         float *kernel_ms /* NULL ok */);

/* ------------------------------------------------------------- cluster boxes */
/* Where each cluster is and how big it is, on the device: what pcl::MomentOfInertiaEstimation (getMassCenter, getAABB,
 * getOBB, getEigenValues, getEigenVectors), pcl::getMinMax3D and pcl::compute3DCentroid give for one cluster at a
 * time, here for every cluster of a member list in one call.  [PCL-upstream: restated from PCL 1.8
 * features/impl/moment_of_inertia_estimation.hpp (computeOBB, the mean and the covariance's eigenvectors) and
 * common/impl/common.hpp (getMinMax3D); no PCL on the build machine]  (tests/boxes_reference.py is the checker).  All
 * arithmetic is as written here, every operation rounded and nothing fused.
 *   members      member e of the list is record indices[e] of pts (indices == NULL: record e); cluster c is members
 *                [offsets[c], offsets[c + 1]).  A member with a non-finite coordinate is skipped and sets
 *                WM_BOX_NONFINITE; n counts the finite members; n == 0 sets WM_BOX_EMPTY and every other field is zero.
 *   aabb         componentwise min and max of the members' floats, ordered by their orderable-integer keys (the sign
 *                bit flipped for a positive float, every bit for a negative one), so -0 < +0.  Exact.
 *   sums         a = aabb_min widened to double; per member d = (double) p - a (every component >= 0); the nine terms
 *                d.x, d.y, d.z, d.x d.x, d.x d.y, d.x d.z, d.y d.y, d.y d.z, d.z d.z are formed in double and each
 *                term t enters as the integer trunc(t * 2^56).  The integers are added exactly: a sum is a function of
 *                the member SET, not of order, wave or workgroup.  A component of aabb_max - a (in double) of 2^20 m or
 *                more sets WM_BOX_RANGE: the moment, axes and OBB fields are zero, n and the AABB stay valid.
 *   centroid,    S1 and S2 are the totals * 2^-56 as doubles (the integer total rounded once); m = S1 / n; centroid =
 *   covariance   (float) (a + m); C = S2 / n - m m^T (the quotient, the product and the difference each rounded).
 *                DEVIATION: PCL sums the uncentred floats in float and subtracts a float mean.
 *   axes         the symmetric eigen-decomposition of C in double (cyclic Jacobi).  Eigenvalues are clamped at 0 and
 *                sorted descending (equal ones keep the order x, y, z of the Jacobi diagonal); major and middle are each
 *                flipped so that their component of largest magnitude is positive (the lowest index on ties); minor =
 *                major x middle.  If the largest eigenvalue is 0 the axes are the identity.  Values and axes are
 *                rounded to float on output.  DEVIATION: PCL leaves the signs to Eigen::EigenSolver.
 *   OBB          PCL's computeOBB on the RETURNED floats of centroid and axes, widened to double: per member e =
 *                (double) p - centroid, s_k = (e.x a_k.x + e.y a_k.y) + e.z a_k.z; lo_k / hi_k the min / max of s_k over
 *                the members; obb_half[k] = (float) ((hi_k - lo_k) / 2); obb_center[i] = (float) (((centroid[i] +
 *                mid_0 a_0[i]) + mid_1 a_1[i]) + mid_2 a_2[i]), mid_k = (hi_k + lo_k) / 2.  Min and max know no order:
 *                given the returned centroid and axes these six floats are exact.
 *   determinism  two calls give identical bytes; permuting the members inside the clusters gives identical bytes. */
typedef struct {                 /* 128 bytes, one per cluster */
    uint32_t n;                  /* finite members */
    uint32_t flags;              /* WM_BOX_* */
    float aabb_min[3], aabb_max[3];
    float centroid[3];
    float eigenvalues[3];        /* of the covariance, descending: major, middle, minor; >= 0 */
    float axes[9];               /* rows: major, middle, minor; orthonormal, right-handed */
    float obb_center[3];         /* PCL getOBB's position */
    float obb_half[3];           /* half extents along the axes (PCL's max_point_OBB) */
    uint32_t reserved[3];        /* zero */
} wm_cluster_box;
enum { WM_BOX_EMPTY = 1, WM_BOX_NONFINITE = 2, WM_BOX_RANGE = 4 };

/* The boxes of n_clusters clusters over n records of `stride_bytes` (x y z first) in `mem`.  offsets has n_clusters + 1
 * entries; `list_mem` says where indices and offsets live, `out_mem` where boxes_out (n_clusters entries) lives.  The
 * call takes wm_cluster_extract's indices_out / offsets_out together with its input cloud, and
 * wm_cluster_extract_batch's points_out / offsets_out with indices == NULL (then n_members must equal n): one call
 * covers the clusters of all scans.  The number of launches and host waits does not depend on n_clusters or n_members.
 * Argument errors, found before a device is touched: a null ctx; with n_clusters > 0 a null offsets / boxes_out; a bad
 * stride, mem, list_mem or out_mem; n, n_members or n_clusters above 0x7FFFFFF0; a null pts with n > 0; indices == NULL with
 * n_members != n.  n_clusters == 0: WM_OK with no device touched.  Found on the device, counted there and brought back
 * in the call's one final fetch: offsets that do not ascend, offsets[0] != 0, offsets[n_clusters] != n_members, an
 * index outside [0, n) -- each gives WM_ERR_ARG with boxes_out unspecified; no kernel reads out of range because of
 * them.  kernel_ms (NULL ok): device time from the upload to the last box.  The workspace is the context's own (freed
 * by wm_ctx_destroy); the registration state and the ground, outlier, cluster and SAC workspaces are not touched. */
int wm_cluster_boxes(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem,
                     const int32_t *indices /* NULL ok */, size_t n_members,
                     const uint32_t *offsets, size_t n_clusters, int list_mem,
                     wm_cluster_box *boxes_out, int out_mem, float *kernel_ms /* NULL ok */);

/* ------------------------------------------------------------- feature descriptors */
/* pcl::FPFHEstimation with a k-neighbourhood (setKSearch) and the nearest-descriptor correspondences of
 * pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33> (determineCorrespondences and
 * determineReciprocalCorrespondences) on the device: what a coarse alignment without an initial pose starts from.
 * [PCL-upstream: restated from PCL 1.8 features/impl/fpfh.hpp and features/impl/pfh_tools.hpp (computePairFeatures);
 * PCL is not linked; tests/fpfh_reference.py is the checker.]
 *
 * All arithmetic is IEEE float32, every operation rounded, nothing fused, in the order written.  A dot product is
 * (x x' + y y') + z z'; a cross-product component is a b - c d; a norm is sqrtf of the dot product; pi is
 * 3.14159274f and 1 / (2 pi) is 0.159154937f.  Everything but atan2f is therefore reproducible bit for bit.
 *   neighbourhood  N(p) = the feature_k nearest points of p's own cloud, p included: the lists of wm_debug_knn (float d2,
 *                  ascending by (d2, index)).  A neighbour with d2 == 0 (p itself, an exact duplicate) is skipped in
 *                  both passes: PCL's `f4 == 0` in the first and `dists == 0` in the second.
 *   pair (p, q)    n_p, n_q: the points' normals, the first three floats of their wm_estimate_normals records or of the
 *                  caller's.  dp = q - p; f4 = |dp|; a1 = (n_p . dp) / f4; a2 = (n_q . dp) / f4.  If fabsf(a1) <
 *                  fabsf(a2) (PCL's acos(fabs(a1)) > acos(fabs(a2))): (n1, n2, dp, f3) = (n_q, n_p, -dp, -a2), else
 *                  (n_p, n_q, dp, a1).  v = dp x n1; |v| == 0: the pair is skipped; v = v / |v| (three divisions).
 *                  w = n1 x v; f2 = v . n2; f1 = atan2f(w . n2, n1 . n2).  A pair with a (0, 0, 0) normal is skipped.
 *   SPFH(p)        three histograms of 11 integer counts; each pair (p, q), q in N(p), that is not skipped adds one to
 *                  bin floorf(11 * ((f1 + pi) * (1 / (2 pi)))) of the first, floorf(11 * ((f2 + 1) * 0.5f)) of the
 *                  second, floorf(11 * ((f3 + 1) * 0.5f)) of the third, each clamped to 0 ... 10.  (PCL adds
 *                  100 / (k - 1) per pair; the factor cancels below.)
 *   FPFH(p)        per block, acc[b] += (float) count_q[b] * (1.0f / d2(p, q)) over q in N(p) in list order (p's own
 *                  SPFH is not added, as in PCL); scale = 100.0f / sum_b acc[b], the sum in bin order, 0 when the sum
 *                  is 0; out[b] = acc[b] * scale.  33 floats per input point in the caller's order: f1's block, f2's,
 *                  f3's.  A non-finite point and a point whose own normal is (0, 0, 0) give 33 zeros (PCL: NaN).
 *   match          d2(i, j) = sum over b = 0 ... 32 of (A[i][b] - B[j][b])^2, accumulated in bin order.  The match of
 *                  row i of A is the row j of B with the smallest (d2, j).  A row of 33 zeros has no match and is
 *                  nobody's match.  Reciprocal: i keeps j only if i is the match of j among A's rows, else -1.  Rows
 *                  must be finite. */
typedef struct {
    int normal_k;   /* neighbours of a normal (normals_in == NULL), 3 ... 32; 0: the default, 10 */
    int feature_k;  /* neighbours of a descriptor, the point itself included, 3 ... 32; 0: the default, 10 */
} wm_fpfh_params;
typedef struct {
    size_t n_valid;    /* finite points whose own normal is not (0, 0, 0): the rows that are not zero by rule */
    float normals_ms;  /* device time of the normals (0 when given or reused) */
    float spfh_ms;     /* ... of the first pass: search, pair features, counts, lists */
    float weight_ms;   /* ... of the second pass: the weighted sums and their scaling */
} wm_fpfh_stats;
void wm_fpfh_default_params(wm_fpfh_params *p);  /* normal_k 10, feature_k 10 */

/* The descriptors of the context's source (which = 0) or target (which = 1), as wm_estimate_normals addresses them.
 * normals_in: NULL = the normals wm_estimate_normals(which, normal_k) gives (the target's are reused when the context
 * holds them for that k, and stay on it); otherwise float x 4 per input point in the caller's order (the fourth float
 * is not read), in `out_mem`'s memory space: PCL's setInputNormals.  fpfh_out: n x 33 floats; spfh_out (NULL ok):
 * n x 33 unsigned char, the first pass's counts in the caller's order, for tests and developers; both in `out_mem`.
 * WM_ERR_ARG: a null ctx or fpfh_out, a k outside 3 ... 32, a bad `which` or `out_mem`.  WM_ERR_STATE without both
 * clouds.  WM_NOT_CONVERGED when the cloud has fewer than feature_k (normals_in == NULL: or normal_k) finite points;
 * nothing is written then.  The workspace is the context's own (freed by wm_ctx_destroy). */
int wm_fpfh_estimate(wm_ctx *ctx, int which, const wm_fpfh_params *params /* NULL: the defaults */,
                     const void *normals_in /* NULL ok */, float *fpfh_out, uint8_t *spfh_out /* NULL ok */, int out_mem,
                     wm_fpfh_stats *stats /* NULL ok */);

/* Normals and descriptors over a RADIUS neighbourhood: pcl::NormalEstimation and pcl::FPFHEstimation with
 * setRadiusSearch, cloud in and rows out (no wm_set_source / wm_set_target), as wm_iss_keypoints.
 * [PCL-upstream: restated from PCL 1.8 features/impl/normal_3d.hpp, common/impl/centroid.hpp
 * (computeMeanAndCovarianceMatrix), features/impl/fpfh.hpp; PCL is not linked; tests/fpfh_radius_reference.py is the
 * checker.]  Float is float32, double is float64, every operation rounded and nothing fused.
 *   neighbours   r2 = (float) (radius * radius), the product in double; r2 must be a normal float > 0.  A neighbour of
 *                finite point i is a finite point j with d2(i, j) < r2 (strict), i itself included; d2 = (dx dx + dy dy)
 *                + dz dz in float, the form every other call uses.  n_s: their number, i included.  A non-finite point
 *                is nobody's neighbour.  r2 = m 2^x with m in [0.5, 1) (frexp), and e = ceil(x / 2).
 *   normal       (viewpoint at the origin) for each neighbour j: d = p_j - p_i, three float subtractions, widened to
 *                double.  Nine integer sums in int64, added exactly: the three first moments rint(d_c 2^(36 - e)) and the
 *                six second moments xx xy xz yy yz zz, rint(d_a d_b 2^(36 - x)) -- the quantum of the keypoints' scatter
 *                sums; rint rounds ties to even.  A term is below about 2^36 and n at most WM_ISS_MAX_POINTS (2^26): no
 *                int64 overflows.  Then in double mean_c = S1_c 2^(e - 36) / n_s and C_ab = S2_ab 2^(x - 36) / n_s -
 *                mean_a mean_b (the products as written: a power of two times the converted sum, divided by n_s), PCL's
 *                single-pass computeMeanAndCovarianceMatrix.  From C to the record exactly as wm_estimate_normals: the
 *                library's svd3 (IEEE operations only), the vector of the smallest value, normalised, negated when
 *                n . p_i > 0, curvature S[2] / (S[0] + S[1] + S[2]); a largest value <= 0 gives (0, 0, 0, 0).  n_s < 3
 *                gives (0, 0, 0, 0) (PCL: NaN).  wm_normal_from_sums is the step from the sums on, on the host.
 *                DEVIATION: PCL adds doubles in its kd-tree's order; a set of integers has one sum.
 *   SPFH(i)      over the neighbours j with 0 < d2 < r2 of the FEATURE radius (d2 == 0, the point itself or an exact
 *                duplicate, is skipped in both passes, as in the k form): the pair features of the k form above, word
 *                for word, with the point's own normal and the neighbour's.  Three histograms of 11 integer counts.
 *                n_f: the number of such neighbours, skipped pairs included; a cloud with n_f > WM_FPFH_RADIUS_MAX_NEIGHBORS
 *                (8191) at some point is outside the call's range.
 *   FPFH(i)      for each such neighbour j: d2c = max(d2, r2 2^-16), ratio = r2 / d2c (a float division; in (1, 65536]),
 *                W = (int64) rint((double) ratio 2^20); acc[b] += count_j[b] W in int64 over the 33 bins (counts <=
 *                8191, neighbours <= 8191, W <= 2^36: acc < 2^62, and so is a block's total).  Per block total = sum_b
 *                acc[b], exact; out[b] = (float) (((double) acc[b] * 100.0) / (double) total); total == 0 gives zeros.
 *                A non-finite point and a point whose own normal is (0, 0, 0) give 33 zeros.  DEVIATIONS from PCL: the
 *                weight is r2 / d2 instead of 1 / d2 (the common factor cancels in the normalisation), quantised to
 *                2^-20 of the weakest weight; a neighbour nearer than r / 256 weighs as one at r / 256; the sum does not
 *                depend on the order.
 *   output       every output byte is a function of the inputs and the parameters: not of the grid's cell (option
 *                "fpfh_cell_div", default 2, 0.5 ... 8: the cell is at least max(normal_radius, feature_radius) /
 *                fpfh_cell_div), nor of the order of the points inside a cell; atan2f sees the same arguments whatever
 *                the order. */
#define WM_FPFH_RADIUS_MAX_NEIGHBORS 8191

/* The normals of a cloud over `radius`.  The cloud (x y z first in each record) lives in `mem`; normals_out (n x 4
 * floats: the unit normal and the curvature), counts_out (n: n_s, -1 for a non-finite point; NULL ok) and sums_out
 * (n x 9 int64: the sums above, zeros for a non-finite point; for tests and developers; NULL ok) live in `out_mem`.
 * Argument errors, found before a device is touched: a null ctx or normals_out; a null cloud with n > 0; a bad stride
 * (< 12 or no multiple of 4), mem or out_mem; n above WM_ISS_MAX_POINTS; a radius that is not finite or whose float
 * square is not a normal float > 0.  n == 0 is WM_OK with no device touched; a cloud without a finite point is WM_OK
 * with zeros.  The workspace is the context's own (freed by wm_ctx_destroy); the registration state and every other
 * workspace stay untouched.  The host waits once in the front (the cloud's box) and once behind the last kernel. */
typedef struct {
    size_t n_finite;
    float kernel_ms;  /* the front to the last kernel */
} wm_normals_radius_stats;
int wm_normals_radius(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, double radius,
                      float *normals_out, int32_t *counts_out /* NULL ok */, int64_t *sums_out /* NULL ok */, int out_mem,
                      wm_normals_radius_stats *stats /* NULL ok */);

/* The step from the nine sums to the record on the host (no device): sums, n_s, x (r2 = m 2^x, -125 <= x <= 128) and
 * the point itself -> out[4].  WM_ERR_ARG: a null argument, a negative n_s, x out of range. */
int wm_normal_from_sums(const int64_t sums[9], int n_s, int x, const float p[3], float out[4]);

typedef struct {
    double normal_radius;   /* read only when normals_in == NULL */
    double feature_radius;
} wm_fpfh_radius_params;
typedef struct {
    size_t n_finite;
    size_t n_valid;        /* finite points whose own normal is not (0, 0, 0) */
    size_t max_neighbors;  /* the largest n_f of the cloud */
    float normals_ms;      /* device time of the normals (0 when given) */
    float spfh_ms;         /* ... of the first walk: pair features and counts */
    float weight_ms;       /* ... of the second walk: the weighted sums and their scaling */
    float kernel_ms;       /* the front to the last kernel */
} wm_fpfh_radius_stats;

/* The descriptors of a cloud.  normals_in: NULL = the normals of wm_normals_radius at normal_radius; otherwise n x 4
 * floats in `mem` in the cloud's order (the fourth is not read): PCL's setInputNormals.  fpfh_out: n x 33 floats;
 * spfh_out (NULL ok): n x 33 uint16, the first walk's counts; counts_out (NULL ok): n entries, n_f, -1 for a non-finite
 * point; all in `out_mem`.  Argument errors as wm_normals_radius (a null params or fpfh_out; feature_radius, and
 * normal_radius when it is read, as `radius` there); n == 0 and a cloud without a finite point likewise.  A point with
 * more than WM_FPFH_RADIUS_MAX_NEIGHBORS feature neighbours: counted on the device and brought back in the call's one
 * final fetch, the call returns WM_ERR_ARG with stats->max_neighbors the true maximum; the outputs are unspecified; no
 * kernel reads or writes out of range because of it. */
int wm_fpfh_radius(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, const wm_fpfh_radius_params *params,
                   const void *normals_in /* NULL ok */, float *fpfh_out, uint16_t *spfh_out /* NULL ok */,
                   int32_t *counts_out /* NULL ok */, int out_mem, wm_fpfh_radius_stats *stats /* NULL ok */);

#define WM_FEATURE_DIM 33
#define WM_FEATURE_MAX_ROWS (1u << 20)
typedef struct {
    size_t n_matched;  /* rows of A with a match (after the reciprocal test) */
    float kernel_ms;   /* device time from the rows' arrival to the last output */
} wm_feature_match_stats;
/* For every one of `na` rows of A its match among the `nb` rows of B (the rule above).  A row is 33 floats at the head
 * of a record of a_stride_bytes / b_stride_bytes (>= 132, a multiple of 4); both arrays in `mem`.  idx_out: int32 x na,
 * d2_out: float x na (NULL ok), in `out_mem`; a row without a match gets -1 and 0.  na, nb <= WM_FEATURE_MAX_ROWS;
 * nb == 0: no row has a match.  Argument errors (a null ctx or idx_out, a null array with rows, a bad stride, mem or
 * out_mem, too many rows) are found before a device is touched; na == 0: WM_OK with no device touched.  The call needs
 * no clouds on the context and touches no registration state. */
int wm_feature_match(wm_ctx *ctx, const void *a, size_t na, size_t a_stride_bytes, const void *b, size_t nb,
                     size_t b_stride_bytes, int mem, int reciprocal, int32_t *idx_out, float *d2_out /* NULL ok */,
                     int out_mem, wm_feature_match_stats *stats /* NULL ok */);

/* ------------------------------------------------------------- pose from correspondences */
/* pcl::registration::CorrespondenceRejectorSampleConsensus on the device: RANSAC over a list of correspondences with
 * SampleConsensusModelRegistration (a rigid transform from three pairs); out come the best transformation and the
 * correspondences it keeps.  The third stage behind wm_fpfh_estimate and wm_feature_match: a pose without a guess.
 * [PCL-upstream: restated from PCL 1.8 registration/impl/correspondence_rejection_sample_consensus.hpp,
 * sample_consensus/sac_model_registration.h and its impl, ransac.hpp; no PCL on the build machine]
 * (tests/corr_ransac_reference.py is the checker).  Float arithmetic is float32, double is float64, every operation
 * rounded and nothing fused; divisions and square roots are the IEEE ones.
 *   input        src (n_src records) and tgt (n_tgt records), x y z first, one stride, in `mem`.  m entries: entry e
 *                pairs source point query_idx[e] (query_idx == NULL: e, and then m <= n_src) with target point
 *                match_idx[e]; both arrays int32 in `mem`.  With query_idx == NULL this is wm_feature_match's idx_out as
 *                it is (-1: no match) and wm_get_correspondences' form.
 *   pairs        an entry is VALID iff both indices are in range and both points are finite.  The valid entries,
 *                ascending by e, are the pairs 0 ... mv - 1.  An invalid entry is labelled WM_CORR_NONE, never counts
 *                and is never sampled.  DEVIATION: PCL samples over all its indices -- a reciprocal match keeps a
 *                tenth of the rows, and a stream over all entries would skip 999 of 1000 triples.
 *   stream       entry j is the plane segmentation's (i0, i1, i2) = sample(seed, j, mv), bit for bit: indices of pairs.
 *   sample test  [isSampleGood]  the three squared distances between the sample's SOURCE points, (dx dx + dy dy) + dz dz
 *                in float for (p0, p1), (p0, p2), (p1, p2), must each be > min_d2.  min_sample_distance >= 0: min_d2 =
 *                the float nearest (double) d * d.  < 0 (the default, -1): [computeSampleDistanceThreshold]
 *                ((sqrt l0 + sqrt l1 + sqrt l2) / 3)^2 with l the eigenvalues of the covariance of the pairs' source
 *                points normalised by mv, clamped at 0.  DEVIATIONS: PCL's float sums are the nine sums in double
 *                relative to pair 0's source point, added exactly (integer limbs, as the plane refit's); the eigenvalues
 *                are the singular values of the one-sided Jacobi SVD on the host; the result is rounded to float, to
 *                nearest; a sum the limbs cannot hold or a non-finite one gives min_d2 = 0.  ADDED: s = |(p1 - p0) x
 *                (p2 - p0)|^2 in float as the plane rule forms it; the entry is SKIPPED iff a distance fails or s is
 *                not finite or not > 0.
 *   hypothesis   [computeModelCoefficients -> estimateRigidTransformationSVD; DEVIATION: its float centroids and
 *                JacobiSVD<Matrix3f> are replaced]  the 17 statistics of wm_umeyama_from_stats in double from the three
 *                pairs in sample order: n = 3, the sums (x0 + x1) + x2, the cross sums (q0a p0b + q1a p1b) + q2a p2b;
 *                then that Umeyama step with no warm start and the IEEE-only one-sided Jacobi SVD.  Its twelve entries
 *                (rows 0 ... 2 of [R | t]) are rounded to float, to nearest; a non-finite entry makes the stream
 *                entry skipped.  wm_corr_hypothesis is this rule on the host.
 *   count        [countWithinDistance]  x' = ((r00 x + r01 y) + r02 z) + tx, y' and z' alike; dx = x' - qx; d2 = (dx dx
 *                + dy dy) + dz dz; a pair is an inlier iff d2 < thr2, thr2 = the smallest float not below (double)
 *                inlier_threshold^2.  A source point matched by several entries counts once per entry (PCL's map keeps
 *                one; with wm_feature_match's output the case does not arise).
 *   loop         the plane segmentation's, with n = mv; an entry is valid or skipped.
 *   no model     mv < 3 (no device work beyond finding mv; none at all with m < 3, or in host memory) or every entry
 *                skipped: WM_NOT_CONVERGED, T_out untouched, *n_out = 0, labels_out not written.
 *   refit        iff refine_model (default 0, PCL's refine_ = false) and the model has >= 3 inliers: the 17 statistics
 *                over the model's inliers in double RELATIVE to the winning sample's first pair (p0, q0), added exactly
 *                (integer limbs); the same Umeyama step on the host; t = q0 + t' - R p0.  T_out is the double result
 *                and the inliers are selected once more with its float rounding.  A sum the limbs cannot hold, or a
 *                non-finite result, keeps the model.  DEVIATION: PCL's refinement loop (re-estimate, shrink the threshold
 *                by the residuals' variance, up to a number of rounds) is not built.
 *   output       T_out: row-major 4 x 4 double on the host; without the refit the winning float entries widened.
 *                inliers_out: the kept entries' positions e, ascending.  labels_out: m bytes.  Every output byte is a
 *                function of the inputs and the parameters; how the stream is cut into rounds (option "corr_round",
 *                default 256, 1 ... 1024) changes nothing but `rounds`. */
typedef struct {
    double inlier_threshold;     /* finite and > 0; PCL's default 0.05 */
    int max_iterations;          /* >= 1; PCL's default 1000 */
    double probability;          /* in (0, 1); 0.99 */
    int refine_model;            /* default 0 */
    double min_sample_distance;  /* finite; < 0 (default -1): from the pairs' source points */
    uint64_t seed;               /* default 0 */
} wm_corr_ransac_params;
void wm_corr_ransac_default_params(wm_corr_ransac_params *p);

enum { WM_CORR_NONE = 0 /* not a valid entry */, WM_CORR_INLIER = 1, WM_CORR_OUTLIER = 2 };
typedef struct {
    size_t n_valid /* mv */, n_inliers_model /* the winning hypothesis' count */, n_inliers /* returned */;
    int iterations, skipped, rounds /* device rounds of the stream */, refined /* the refit replaced the model */;
    long long hypotheses /* stream entries consumed */, best_hypothesis /* its stream index, -1: none */;
    float min_d2;     /* the sample test's bound as it was applied */
    float model[12];  /* the winning hypothesis before the refit */
    float kernel_ms;  /* the front to the last output */
} wm_corr_ransac_stats;

/* T_out (host, 16 doubles).  inliers_out (cap entries) and labels_out (m bytes, WM_CORR_*) live in `out_mem`.  More
 * inliers than `cap`: WM_ERR_ARG with the first `cap` written and *n_out the true count.  Argument errors, found
 * before a device is touched: a null ctx / params / T_out / n_out; a bad stride (< 12 or no multiple of 4), mem or
 * out_mem; n_src or n_tgt above 0x7FFFFFF0; m above WM_FEATURE_MAX_ROWS; query_idx == NULL with m > n_src; a null
 * cloud with records; a null match_idx with m > 0; a null inliers_out with cap > 0; and the parameter ranges above.
 * The workspace is the context's own (freed by wm_ctx_destroy); the registration state and every other workspace stay
 * untouched. */
int wm_corr_ransac(wm_ctx *ctx, const void *src, size_t n_src, const void *tgt, size_t n_tgt, size_t stride_bytes,
                   const int32_t *query_idx /* NULL ok */, const int32_t *match_idx, size_t m, int mem,
                   const wm_corr_ransac_params *params, double T_out[16], int32_t *inliers_out, size_t cap, int out_mem,
                   size_t *n_out, uint8_t *labels_out /* NULL ok */, wm_corr_ransac_stats *stats /* NULL ok */);

/* The hypothesis rule on the host (no device): p and q are the sample's three source and target points, x y z each, in
 * sample order.  Returns 1 with T_out = the twelve floats, or 0 (skipped) with T_out zero; negative: a null argument. */
int wm_corr_hypothesis(const float p[9], const float q[9], float min_d2, float T_out[12]);

/* For tests and developers: entries j0 ... j0 + count - 1 (count <= 1024) of the hypothesis stream of the LAST
 * wm_corr_ransac call on this context (its pairs, seed and min_d2), evaluated by the device: twelve floats and a flag
 * (1 valid, 0 skipped) per entry, host memory.  WM_ERR_STATE without such a call or with fewer than 3 pairs. */
int wm_debug_corr_hypotheses(wm_ctx *ctx, uint64_t j0, int count, float *T_out, uint32_t *flags_out);

/* ------------------------------------------------------------- keypoints */
/* pcl::ISSKeypoint3D on the device: the few points of a cloud worth matching, in front of wm_feature_match (describe
 * all points, keep the keypoints' rows with wm_gather_records, match those).
 * [PCL-upstream: restated from PCL 1.8 keypoints/impl/iss_3d.hpp, getScatterMatrix and detectKeypoints; no PCL on the
 * build machine] (tests/iss_reference.py is the checker).  Float is float32, double is float64, every operation
 * rounded and nothing fused.
 *   neighbours   r2s = (float) (salient_radius * salient_radius), r2n = (float) (non_max_radius * non_max_radius), the
 *                products in double.  A neighbour of finite point i is a finite point j with d2(i, j) < r2 (strict, as
 *                FLANN's radius set), i itself included; d2 = (dx dx + dy dy) + dz dz in float, the form every other
 *                call uses.  A non-finite point is nobody's neighbour and gets WM_ISS_NONE.
 *   scatter      for each neighbour j within r2s: d = p_j - p_i, three float subtractions, widened (as PCL); the six
 *                products dx dx, dx dy, dx dz, dy dy, dy dz, dz dz in double (exact: 24 + 24 bits).  Each enters its
 *                sum as the integer rint(product * scale), ties to even, scale = 2^(36 - x) with r2s = m 2^x, m in
 *                [0.5, 1) (frexp); the integers are added exactly in int64.  DEVIATION: PCL adds the doubles in its
 *                kd-tree's order; here the sum must not depend on the order of the points inside a grid cell, and a
 *                set of integers has one sum.  The quantum is 2^-36 of r2s; a term is below about 2^36 and n is at
 *                most WM_ISS_MAX_POINTS (2^26), so an int64 cannot overflow.  n_s: the number of neighbours, i included.
 *   saliency     n_s < min_neighbors: third = 0.  Otherwise the six sums, converted to double (round to nearest), form
 *                the symmetric matrix; its eigenvalues by cyclic Jacobi sweeps (the library's jacobi3), sorted l1 >= l2
 *                >= l3.  Point i is SALIENT iff the three are finite, l3 > 0, l2 / l1 < gamma_21 and l3 / l2 < gamma_32
 *                (divisions in double; a NaN fails).  A salient point has third = ldexp(l3, x - 36), every other point
 *                third = 0.  wm_iss_third is this step on the host.  DEVIATIONS: the Jacobi sweeps stand in for Eigen's
 *                SelfAdjointEigenSolver; PCL leaves a stale thread-local value behind when it skips a point with l3 < 0
 *                or a non-finite value -- here such a point is simply not salient; there is no border estimation
 *                (border_radius, normal_radius and angle_threshold do not exist).
 *   suppression  point i is a KEYPOINT iff third_i > 0, the number of its neighbours within r2n (i included) is >=
 *                min_neighbors, and no such neighbour j has third_j > third_i (strict).  Equal values survive together,
 *                as PCL's `<` test leaves them (exact duplicates are the case that arises).
 *   output       the keypoints' caller indices, ascending (PCL's order).  Every output byte is a function of the inputs
 *                and the parameters: not of the grid's cell (option "iss_cell_div", default 2, 0.5 ... 8: the cell is
 *                at least max(salient_radius, non_max_radius) / iss_cell_div), nor of the order of rows that are not
 *                compared. */
typedef struct {
    double salient_radius;   /* finite, (float) r^2 a normal float > 0; no usable default: 0 */
    double non_max_radius;   /* the same */
    double gamma_21;         /* finite, >= 0; 0.975 */
    double gamma_32;         /* finite, >= 0; 0.975 */
    int min_neighbors;       /* >= 0; 5 */
} wm_iss_params;
void wm_iss_default_params(wm_iss_params *p);

typedef struct {
    size_t n_finite, n_salient, n_keypoints;
    float kernel_ms;  /* the front to the keypoint list */
} wm_iss_stats;

enum { WM_ISS_NONE = 0 /* non-finite */, WM_ISS_PLAIN = 1, WM_ISS_SALIENT = 2 /* third > 0, suppressed */, WM_ISS_KEYPOINT = 3 };
#define WM_ISS_MAX_POINTS 0x4000000ull /* n at most: 2^26 */

/* The cloud (x y z first in each record) lives in `mem`; indices_out (cap entries), labels_out (n bytes, WM_ISS_*),
 * third_out (n doubles; 0 for a point that is not salient) and counts_out (n: n_s, -1 for a non-finite point) live in
 * `out_mem`.  More keypoints than `cap`: WM_ERR_ARG with the first `cap` written and *n_out the true count.  A cloud
 * without a finite point, or without a keypoint, is WM_OK with *n_out = 0.  Argument errors, found before a device is
 * touched: a null ctx / params / n_out; a null cloud with n > 0; a bad stride (< 12 or no multiple of 4), mem or
 * out_mem; n above WM_ISS_MAX_POINTS; a null indices_out with cap > 0; and the parameter ranges above.  n == 0 is
 * WM_OK with no device touched.  The workspace is the context's own (freed by wm_ctx_destroy); the registration state
 * and every other workspace stay untouched.  The counters come back in one copy behind the last kernel, and the host
 * waits there (and once in the front, for the cloud's box, as wm_outlier_filter). */
int wm_iss_keypoints(wm_ctx *ctx, const void *pts, size_t n, size_t stride_bytes, int mem, const wm_iss_params *p,
                     int32_t *indices_out, size_t cap, int out_mem, size_t *n_out, uint8_t *labels_out /* NULL ok */,
                     double *third_out /* NULL ok */, int32_t *counts_out /* NULL ok */, wm_iss_stats *stats /* NULL ok */);

/* The saliency step on the host (no device): the six integer sums (xx xy xz yy yz zz), n_s and x (r2s = m 2^x, -125
 * <= x <= 128) -> *third_out.  Of `p` only gamma_21, gamma_32 and min_neighbors are read.  WM_ERR_ARG: a null
 * argument, x or one of those three out of range. */
int wm_iss_third(const int64_t sums[6], int n_s, int x, const wm_iss_params *p, double *third_out);

/* Record j of dst = record idx[j] of src (n records of stride_bytes, a multiple of 4 up to WM_GATHER_MAX_STRIDE), j <
 * m; src, idx and dst all live in `mem` and do not overlap.  It selects the keypoints' rows of wm_fpfh_estimate's
 * output for wm_feature_match.  An index outside [0, n) gives WM_ERR_ARG: nothing is read out of range, that record of
 * dst is not written (host memory: nothing is written at all).  n and m at most 0x7FFFFFF0; m == 0 is WM_OK with no
 * device touched.  Device memory: one kernel, one counter back. */
#define WM_GATHER_MAX_STRIDE 65536u
int wm_gather_records(wm_ctx *ctx, const void *src, size_t n, size_t stride_bytes, const int32_t *idx, size_t m,
                      void *dst, int mem);

/* All ranks in ONE process: one context and one worker thread per device, RCCL communicators from
 * ncclCommInitAll (emulate != 0: `n_devices` ranks on devices[0] with the host stand-in exchange).
 * wm_multi_icp_align runs one sharded registration of two HOST clouds (uploaded once, broadcast over
 * xGMI) and returns rank 0's result; wm_multi_icp_match is ICPMatcher::match() with its voxel filter
 * and scales; wm_multi_icp_info the estimators after either. */
typedef struct wm_multi wm_multi;
int wm_multi_create(wm_multi **out, const int *devices, int n_devices, int emulate);
void wm_multi_destroy(wm_multi *m);
int wm_multi_size(const wm_multi *m);
int wm_multi_icp_align(wm_multi *m, const void *ref, size_t n_ref, const void *target, size_t n_target,
                       size_t stride_bytes, const wm_icp_params *p, double T_out[16], wm_icp_stats *stats);
int wm_multi_icp_match(wm_multi *m, const void *ref, size_t n_ref, const void *target, size_t n_target,
                       size_t stride_bytes, const wm_icp_params *p, float res, int multiscale_steps,
                       double T_out[16], wm_icp_stats *stats);
int wm_multi_icp_info(wm_multi *m, int method, const double T_result[16], double lin_covar, double ang_covar,
                      double max_corr, double info_out[36], int *degenerate);

/* Host-only twin of the per-iteration solve + PCL stopping rules (no GPU touched):
 * the very function the device runs after the all-reduce, callable on the CPU so
 * that the sharded control flow can be exercised without a GPU. */
typedef struct wm_host_icp wm_host_icp;
int wm_host_icp_create(wm_host_icp **out, const wm_icp_params *p, size_t expect_owned_total);
void wm_host_icp_destroy(wm_host_icp *h);
int wm_host_icp_apply(wm_host_icp *h, const double stats[WM_STATS_LEN]);
int wm_host_icp_get(const wm_host_icp *h, int *done, double T_out[16], wm_icp_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* WAVEMATCH_H */
