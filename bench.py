#!/usr/bin/env python3
"""bench.py -- BASELINE.json's headline metric on MI355X.

  metric : point-cloud registrations/sec (1M<->1M pts, ICP, 50 iterations)
  step   : ONE full registration through the C ABI with both clouds already resident
           in HBM ("device-resident"): wm_set_source (pack, Morton order) + wm_set_target
           (pack, grid ladder) + wm_icp_align (50 forced iterations: correspondence search
           with the iteration's statistics fused into its tail, row reduction, Umeyama
           solve, all on device).  The same registration from HOST clouds (H2D inside the
           step, pageable and pinned) is reported beside it in config.host_clouds; it is
           never `value`.
  N > 1  : one process per GPU (launched plainly, `python bench.py --gpus N` re-executes itself under
           torch.distributed.run on 127.0.0.1).  The registration is sharded INSIDE the library
           (wm_icp_align_sharded, libwave_amd/csrc/wm_shard.hip): slab planning on the
           device, the iteration loop in C++, one exchange of 34 doubles per iteration (the
           ranks' mailboxes over xGMI, summed inside the solve kernel; ncclAllReduce on the
           context's stream where mailboxes cannot be set up).  torch.distributed only carries
           the 128-byte RCCL id to the ranks and the barriers around the timed region.
           Weak scaling: N x 1M points per cloud.

Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype, ms_per_step, ... and "roofline"
(correspondence kernel vs the HBM roof, from the timed steps' event-bracketed launches and the committed counter capture).
A plain run sets up, warms up, times --steps registrations and prints that line.

--full adds every other measurement, each a run of its own after the timed steps: "config.host_clouds"
(the step from pageable / pinned host clouds), "in_flight" (several registrations in flight),
"other_configs" (BASELINE configs[2] GICP 500k, configs[3] NDT 2M, configs[0] 10k pairs in batches of
256, and default-parameter matches of 55k pairs in batches of 128), "cpu_baseline" (the CPU oracle timed
on this box's host cores: 1 core, and the MultiMatcher pattern on all usable cores) -- N == 1 only --,
the device's copy rate (roofline.hbm_util) and, at N > 1, the isolated all-reduce and the second timing
with the collective exchange.  The --no-* options leave single parts of --full out.

--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (float64 / float32).
"""
import argparse
import json
import os

# One process per GPU: keep numpy / torch CPU thread pools small.  Their default is one thread per
# logical CPU (256 here); the pools' spinning workers burn the container's CPU quota during set-up
# and the whole process is then throttled for tens of milliseconds somewhere in the timed region
# (cgroup cpu.stat: nr_throttled) -- seen as one 50-90 ms registration per run.
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")
# multi-process GPU work on these hosts needs dmabuf IPC (RCCL's hipIpcGetMemHandle fails otherwise); the
# driver's environment exports it -- kept here too, for a launch line that does not
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s copy-measured)
VALU_ISSUE_PEAK_GINST = 256 * 4 * 2.4 / 4.0  # G wave64 VALU instructions/s: 1024 SIMDs, one issue per 4 cycles at 2.4 GHz (MI355X_MICROARCH.md)
F64_VALU_PEAK_TFLOPS = 78.6  # MI355X vector FP64 (half the 157.3 TFLOP/s FP32 vector rate)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed registrations")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=1_000_000, help="points per cloud PER GPU")
    ap.add_argument("--iters", type=int, default=50, help="forced ICP iterations per registration")
    ap.add_argument("--max-corr", type=float, default=3.0)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run every other measurement too (host clouds, registrations in flight, "
                         "other configs, CPU baselines, the device's copy rate; at N > 1 the collective exchange)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip the other configs")
    ap.add_argument("--no-in-flight", action="store_true",
                    help="with --full: skip the several-registrations-in-flight measurement")
    ap.add_argument("--no-host-clouds", action="store_true",
                    help="with --full: skip the H2D-inclusive steps (counter captures: the process then ends with the timed registrations)")
    ap.add_argument("--cpu-iters", type=int, default=20, help="oracle iterations timed for the baseline")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


DUMP_MAX_POINTS = 2_000_000  # per-point outputs above this are dumped as a fixed, seeded sample (at most 20 B a point)


def dump_outputs(out_dir, r, ctx=None):
    """What the last timed step computed, as `out_dir`/<name>.npy: the registration's transform and the statistics
    wm_icp_align returns (float64) and, from a single-GPU context, the last iteration's correspondences -- matched
    target index (float64, -1 = none) and squared distance (float32) per source point, in source order.  Clouds of
    more than DUMP_MAX_POINTS points leave a sample of that many source points (seed 0, ascending; indices in
    correspondence_sample.npy)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"transform": np.asarray(r["T"], dtype=np.float64)}
    for k in ("iterations", "n_corr", "mse", "prev_mse", "converged"):
        arrays[k] = np.asarray(float(r[k]), dtype=np.float64)
    if ctx is not None:
        idx, d2 = ctx.correspondences()
        if len(idx) > DUMP_MAX_POINTS:
            pick = np.sort(np.random.default_rng(0).choice(len(idx), DUMP_MAX_POINTS, replace=False))
            idx, d2 = idx[pick], d2[pick]
            arrays["correspondence_sample"] = pick.astype(np.float64)
        arrays["correspondence_index"] = idx.astype(np.float64)
        arrays["correspondence_d2"] = d2.astype(np.float32)
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), v)
    return sorted(arrays)


def first_step_with_fallback(step, rebuild, all_ranks_ok, error_type):
    """The first sharded registration of a run, on every rank: if it fails on ANY rank (`all_ranks_ok` is a collective
    AND over the ranks), every rank calls `rebuild` (collective) and the registration is tried once more; a second
    failure is raised.  Returns True when the fallback was taken."""
    err = None
    try:
        step()
    except error_type as e:
        err = e
    if all_ranks_ok(err is None):
        return False
    rebuild()
    err2 = None
    try:
        step()
    except error_type as e:
        err2 = e
    if not all_ranks_ok(err2 is None):
        raise RuntimeError("sharded registration failed with the collective exchange too: %s (first: %s)" % (err2, err))
    return True


def usable_cpus():
    """CPUs this process may really use: the affinity mask, cut by the container's CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:
        pass
    return n


def cpu_description():
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    flags = "unknown"
    try:
        for line in open(os.path.join(ROOT, "oracle", "Makefile")):
            if line.startswith("CFLAGS"):
                flags = line.split("=", 1)[1].strip()
    except Exception:
        pass
    return {"cpu_model": model, "logical_cpus": os.cpu_count(), "usable_cpus": usable_cpus(),
            "compiler": "gcc", "flags": flags}


def cpu_baseline(ref, tgt, iters_full, max_corr, cpu_iters):
    """The CPU oracle (oracle/: kd-tree exact NN + Umeyama, single thread like PCL) on a bounded
    sample of the same workload.  (i) one core: tree build + `cpu_iters` iterations timed, scaled to
    the `iters_full`-iteration registration.  (ii) the reference's own parallelism -- MultiMatcher,
    one independent registration per thread (multi_matcher.hpp:32) -- on all usable cores: every
    thread builds its tree and runs 2 iterations of the same pair at the same time (memory-bandwidth
    and cache contention included), scaled the same way."""
    from oracle import oracle_py as O
    O.lib()
    t0 = time.perf_counter()
    O.KdTree(tgt)
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    O.icp_align(ref, tgt, max_corr=max_corr, force_iterations=cpu_iters)
    t_run = time.perf_counter() - t0
    per_iter = max(t_run - t_build, 1e-9) / cpu_iters
    t_full = t_build + per_iter * iters_full
    out = {
        "value": 1.0 / t_full, "unit": "registrations/s", "cores": 1, "kind": "port",
        "sample": "same %d<->%d clouds; kd-tree build (%.2f s) + %d of %d iterations timed "
                  "(%.3f s/iter), scaled to %d iterations" % (len(ref), len(tgt), t_build,
                                                              cpu_iters, iters_full, per_iter,
                                                              iters_full),
        "seconds_per_registration": t_full, "host": cpu_description(),
    }
    nthr = usable_cpus()
    if nthr > 1:
        it_a, it_b = 1, 3
        walls = {}

        def worker(k, iters):
            t = time.perf_counter()
            O.icp_align(ref, tgt, max_corr=max_corr, force_iterations=iters)
            walls[(k, iters)] = time.perf_counter() - t
        for iters in (it_a, it_b):
            th = [threading.Thread(target=worker, args=(k, iters)) for k in range(nthr)]
            [t.start() for t in th]
            [t.join() for t in th]
        wa = float(np.mean([walls[(k, it_a)] for k in range(nthr)]))
        wb = float(np.mean([walls[(k, it_b)] for k in range(nthr)]))
        it_c = max((wb - wa) / (it_b - it_a), 1e-9)   # one iteration, all cores busy
        build_c = max(wa - it_a * it_c, 0.0)           # one tree build, all cores busy
        t_reg = build_c + it_c * iters_full
        out["all_cores"] = {
            "value": nthr / t_reg, "unit": "registrations/s", "cores": nthr,
            "pattern": "MultiMatcher: one independent registration per thread, %d threads" % nthr,
            "sample": "every thread: tree build + %d, then + %d iterations of the same pair, concurrently; "
                      "%.2f s build, %.3f s/iter under load, scaled to %d iterations" % (it_a, it_b, build_c, it_c,
                                                                                        iters_full),
            "seconds_per_registration_per_thread": t_reg,
        }
    return out


def rotation_angle(R_a, R_b):
    """Angle [rad] of R_a^T R_b through |R - I|_F = 2 sqrt(2) |sin(theta / 2)|: well conditioned near zero, where
    arccos((trace - 1) / 2) turns the 1e-7 non-orthonormality of a float matrix into 3e-4 rad (tests/helpers.py:
    pose_error is the same formula)."""
    R = np.asarray(R_a, dtype=np.float64).T @ np.asarray(R_b, dtype=np.float64)
    return float(2.0 * np.arcsin(min(1.0, np.linalg.norm(R - np.eye(3)) / (2.0 * np.sqrt(2.0)))))


def csrc_sha256():
    """sha256 over the kernel sources (libwave_amd/csrc/*.hip, *.hpp, in name order): what a committed counter
    capture is stamped with (scripts/pmc_to_json.py) and checked against here."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "libwave_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".hpp")):
            h.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def pmc_summary():
    """Committed PMC summary of this bench command (profiles/pmc_latest.json, written by
    scripts/gpu_pmc.sh + scripts/pmc_to_json.py from separate rocprofv3 --pmc passes).  A capture whose
    source stamp differs from the kernels in the tree is STALE: it is returned empty (every `traffic` /
    `hbm_util` derived from it becomes null) with the reason under "stale"."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_latest.json")) as f:
            pmc = json.load(f)
    except Exception:
        return {}
    stamp = pmc.get("csrc_sha256")
    if stamp is None:  # (an unstamped capture cannot be tied to the kernels in the tree: treated as stale too)
        return {"stale": "profiles/pmc_latest.json (tag %s) carries no csrc_sha256 stamp: traffic not reported" % pmc.get("tag")}
    if stamp != csrc_sha256():
        return {"stale": "profiles/pmc_latest.json (tag %s) was captured from other kernel sources "
                         "(csrc_sha256 %s..., tree %s...): traffic not reported" % (pmc.get("tag"), stamp[:12],
                                                                                   csrc_sha256()[:12])}
    return pmc


def pmc_traffic_bytes(pmc, kernel="k_nn_grid", stream_bytes=None):
    """HBM bytes per launch of a kernel from its FETCH_SIZE / WRITE_SIZE counters.  What FETCH_SIZE counts was
    calibrated on this part with access patterns of known traffic (scripts/gpu_fetch_calib.sh ->
    profiles/r04_fetch_size_calibration.json): a wide coalesced stream is tallied at HALF its bytes (2 GiB read =
    1024 MiB counted: the guide's gfx950 note), a gather is tallied at what it moves -- 64 B per lone 16-byte
    element, 128 B (the whole line) per run of four float4, the unit of the search's candidate walk.  So
      stream_bytes = None : a streaming kernel, 2 x FETCH + WRITE;
      stream_bytes = S    : a kernel that reads S bytes in coalesced streams and gathers the rest:
                            (FETCH - S / 2) for the gathers + S for the streams = FETCH + S / 2, + WRITE."""
    d = pmc.get(kernel)
    if not d or "FETCH_SIZE_kb_per_dispatch" not in d:
        return None
    fetch, write = d["FETCH_SIZE_kb_per_dispatch"] * 1024.0, d["WRITE_SIZE_kb_per_dispatch"] * 1024.0
    if stream_bytes is None:
        return 2.0 * fetch + write
    return max(fetch + 0.5 * stream_bytes, stream_bytes) + write


def counter_traffic(pmc, kernel, avg_launch_us, copy_peak_gbs):
    """HBM bytes per launch of `kernel` from the committed PMC passes (profiles/pmc_latest.json; FETCH_SIZE
    doubled on gfx950 as for the search kernels, WRITE_SIZE as reported) and, with the launch time measured
    in THIS run, the share of the measured copy rate they amount to."""
    d = pmc.get(kernel, {})
    if "FETCH_SIZE_kb_per_dispatch" not in d or "WRITE_SIZE_kb_per_dispatch" not in d:
        return {"traffic": None}
    t = (2.0 * d["FETCH_SIZE_kb_per_dispatch"] + d["WRITE_SIZE_kb_per_dispatch"]) * 1024.0
    out = {"traffic": t, "traffic_source": "profiles/pmc_latest.json, %s" % d.get("traffic_source", pmc.get("tag"))}
    if avg_launch_us and avg_launch_us > 0 and copy_peak_gbs:
        out["hbm_util"] = t / (avg_launch_us * 1e-6) / 1e9 / copy_peak_gbs
    return out


def other_configs(torch, dev, capi, synth, pmc, with_cpu, copy_peak=None):
    """BASELINE configs[2] (GICP 500k<->500k) and configs[3] (NDT 2M, 0.5 m voxels): ms per
    registration (device-resident clouds), the dominant kernel against its roof, and the CPU oracle
    at a size it finishes in seconds."""
    out = []
    os.environ["WM_GICP_PROFILE"] = "1"
    os.environ["WM_NDT_PROFILE"] = "1"
    prof = capi.Context(0)   # event timing around every objective / derivative kernel (slower host side)
    del os.environ["WM_GICP_PROFILE"], os.environ["WM_NDT_PROFILE"]
    ctx = capi.Context(0)

    def median_ms(fn, reps=7, warm=3):
        # (the first registrations of a workload in a process are 5-8 % slower than the ones behind them -- buffers growing
        # to size, clocks: scripts/bench_configs.py lists every repetition --; the median is over the ones behind them)
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), r

    # ---- configs[2]
    n = 500_000
    ref, tgt, T_gt = synth.pair(n, seed=42)
    d_ref, d_tgt = torch.from_numpy(ref).to(dev), torch.from_numpy(tgt).to(dev)

    def gicp(c, **kw):
        c.set_source(d_ref)
        c.set_target(d_tgt)
        return c.gicp_align(**kw)
    # the default = the REFERENCE's algorithm: PCL's per-pair sums (one pass over the pairs per evaluation; answered by the
    # resident evaluator k_gicp_fdf_served, trial points through a mailbox the host writes over the PCIe BAR) ...
    PCL, STAT = capi.WM_GICP_OBJECTIVE_PCL_SUMS, capi.WM_GICP_OBJECTIVE_STATISTICS
    assert capi.gicp_params().objective == PCL
    ms_pcl, r_pcl = median_ms(lambda: gicp(ctx))
    rp_pcl = gicp(prof)
    launched = capi.Context(0)
    launched.set_option("gicp_served", 0)
    ms_launched, _ = median_ms(lambda: gicp(launched))   # ... or with a kernel launch per evaluation
    launched.close()
    # ... and the opt-in: the objective as 74 sufficient statistics per outer iteration (csrc/wm_gicp_quad.hpp) -- NOT PCL's
    # arithmetic (its registrations of noisy pairs end up to 1e-3 m from PCL's: tests/test_gicp_quad_gpu.py)
    ms, r = median_ms(lambda: gicp(ctx, objective=STAT))
    rp = gicp(prof, objective=STAT)
    passes = max(rp["iterations"], 1)
    us = rp["fdf_kernel_ms"] / passes * 1e3
    bytes_pass = 184.0 * n  # 16 source point + 8 key + 16 match + 72 source covariance + 72 target covariance (gathered)
    ev = max(rp_pcl["evaluations"], 1)
    us_fdf = rp_pcl["fdf_kernel_ms"] / ev * 1e3
    bytes_eval = 112.0 * n  # 16 source + 16 match + 8 key + 72 Mahalanobis per pair
    e = {"config": "GICPMatcher 500k<->500k, k = 10 covariances (BASELINE configs[2])",
         # the driver-visible pair the verdict asked for: the default's time, the reference algorithm's time (the same
         # thing since round 6: the default IS the reference's algorithm) and the opt-in's
         "ms_per_registration": ms_pcl, "ms_per_registration_pcl_sums": ms_pcl, "ms_per_registration_statistics": ms,
         "reference_algorithm": "pcl_sums (the default: wm_gicp_params::objective = WM_GICP_OBJECTIVE_PCL_SUMS = 0; "
                                "wave_matching/src/gicp.cpp:58 -> PCL's OptimizationFunctorWithIndices)",
         "registrations_per_s": 1e3 / ms_pcl, "outer_iterations": r_pcl["iterations"],
         "objective_evaluations": r_pcl["evaluations"], "served_evaluations": r_pcl.get("served_evaluations"),
         "ms_per_registration_launched": ms_launched,
         "objective": "PCL's per-pair sums through the float transform at every trial point of the line search",
         "translation_error_m": float(np.linalg.norm(r_pcl["T"][:3, 3] - T_gt[:3, 3])) if r_pcl["T"] is not None else None,
         "roofline": {"bound": "hbm", "kernel": "wm::k_gicp_fdf (one per BFGS evaluation, timed as launched kernels)",
                      "achieved": bytes_eval / (us_fdf * 1e-6) / 1e9 if us_fdf > 0 else None, "peak": HBM_PEAK_GBS,
                      "unit": "GB/s", "frac": bytes_eval / (us_fdf * 1e-6) / 1e9 / HBM_PEAK_GBS if us_fdf > 0 else None,
                      "algorithmic_bytes_per_launch": bytes_eval, "avg_launch_us": us_fdf, "launches_timed": ev,
                      # SURVEY 8(d)'s accounting of one objective evaluation: 52 B x n
                      "survey_bytes_per_launch": 52.0 * n,
                      "frac_survey_bytes": 52.0 * n / (us_fdf * 1e-6) / 1e9 / HBM_PEAK_GBS if us_fdf > 0 else None},
         "statistics": {"ms_per_registration": ms, "registrations_per_s": 1e3 / ms, "outer_iterations": r["iterations"],
                        "objective_evaluations": r["evaluations"],
                        "objective": "OPT-IN, not the reference's arithmetic: 74 sufficient statistics per outer iteration, every "
                                     "evaluation scalar work on the host (WM_GICP_OBJECTIVE_STATISTICS = 1; "
                                     "GICPMatcher::setObjective / WAVE_GICP_OBJECTIVE=statistics)",
                        "translation_error_m": float(np.linalg.norm(r["T"][:3, 3] - T_gt[:3, 3])) if r["T"] is not None else None,
                        "difference_to_the_default_m": (float(np.linalg.norm(r["T"][:3, 3] - r_pcl["T"][:3, 3]))
                                                        if r["T"] is not None and r_pcl["T"] is not None else None),
                        "roofline": {"bound": "hbm", "kernel": "wm::k_gicp_quad (ONE pass over the pairs per outer iteration: Mahalanobis "
                                                               "matrices formed on the fly, 74 double-double sums; both halves of the sums read the pairs)",
                                     "achieved": bytes_pass / (us * 1e-6) / 1e9 if us > 0 else None, "peak": HBM_PEAK_GBS,
                                     "unit": "GB/s", "frac": bytes_pass / (us * 1e-6) / 1e9 / HBM_PEAK_GBS if us > 0 else None,
                                     "algorithmic_bytes_per_launch": bytes_pass, "avg_launch_us": us, "launches_timed": passes}}}
    try:
        e["in_flight"] = two_in_flight(torch, capi, gicp)
    except Exception as ex:
        e["in_flight"] = {"error": str(ex)}
    e["roofline"].update(counter_traffic(pmc, "k_gicp_fdf", us_fdf, copy_peak))
    e["statistics"]["roofline"].update(counter_traffic(pmc, "k_gicp_quad", us, copy_peak))
    if with_cpu:
        from oracle import oracle_py as O
        m = 20_000
        rs, ts_, _ = synth.pair(m, seed=42)
        t0 = time.perf_counter()
        want_pcl = O.gicp_align(rs, ts_)
        e["cpu_baseline"] = {"seconds_per_registration": time.perf_counter() - t0, "cores": 1, "kind": "port",
                             "sample": "the oracle's GICP (PCL's per-pair objective) on a %d<->%d pair of the same scene "
                                       "(the 500k pair takes minutes)" % (m, m)}
        O.gicp_set_objective(1)   # (the oracle's restatement of the builder's reformulation: what the opt-in is held to)
        try:
            want = O.gicp_align(rs, ts_)
        finally:
            O.gicp_set_objective(0)
        # parity where the oracle can be run: the SAME 20k pair through the HIP path.  (translation_error_m above
        # is against the ground truth of a noisy re-sampled pair -- what GICP's loose BFGS stop leaves, for the
        # oracle as for the kernels -- not a difference between the two.)
        try:
            ctx.set_source(rs)
            ctx.set_target(ts_)
            got_p = ctx.gicp_align()
            Tp = np.asarray(want_pcl["T"], dtype=np.float64)
            e["parity_vs_oracle_20k"] = {
                "translation_difference_m": float(np.linalg.norm(got_p["T"][:3, 3] - Tp[:3, 3])) if got_p["T"] is not None else None,
                "rotation_difference_rad": rotation_angle(got_p["T"][:3, :3], Tp[:3, :3]) if got_p["T"] is not None else None,
                "identical_float_matrix": bool(got_p["T"] is not None and np.array_equal(got_p["T"].astype(np.float32), Tp.astype(np.float32))),
                "outer_iterations": [got_p["iterations"], want_pcl.get("iterations")],
                "note": "the same 20k pair through the HIP path (default objective: PCL's per-pair sums) and the oracle's default "
                        "mode (its restatement of PCL's GICP); translation_error_m above is against the ground truth of the "
                        "noisy 500k pair, not a parity figure"}
            got = ctx.gicp_align(objective=STAT)
            if got["T"] is not None and want.get("T") is not None:
                Tw = np.asarray(want["T"], dtype=np.float64)
                e["parity_vs_oracle_20k"]["statistics"] = {
                    "identical_float_matrix_vs_the_oracles_restatement_of_the_reformulation":
                        bool(np.array_equal(got["T"].astype(np.float32), Tw.astype(np.float32))),
                    "statistics_vs_pcl_sums_translation_difference_m": float(np.linalg.norm(got["T"][:3, 3] - Tp[:3, 3])),
                    "statistics_vs_pcl_sums_rotation_difference_rad": rotation_angle(got["T"][:3, :3], Tp[:3, :3]),
                    "note": "the opt-in objective against the oracle's objective mode 1 (a restatement check, not reference parity), "
                            "and how far its registration of this noisy pair is from the default's (PCL's BFGS stops at |g| < 1e-2 "
                            "wherever its line search lands: tests/test_gicp_quad_gpu.py)"}
        except Exception as ex:  # (never lose the line over the extra check)
            e["parity_vs_oracle_20k"] = {"error": str(ex)}
    out.append(e)
    del d_ref, d_tgt

    # ---- configs[3]
    n = 2_000_000
    ref, tgt, T_gt = synth.pair(n, seed=42, pattern="rings")
    d_ref, d_tgt = torch.from_numpy(ref).to(dev), torch.from_numpy(tgt).to(dev)

    def ndt(c):
        c.set_source(d_ref)
        c.set_target(d_tgt)
        return c.ndt_align(res=0.5)
    ms, r = median_ms(lambda: ndt(ctx))
    rp = ndt(prof)
    ev = max(rp["evaluations"], 1)
    us = rp["deriv_kernel_ms"] / ev * 1e3
    e = {"config": "NDTMatcher 2M-point 64-ring scan pair, 0.5 m voxels (BASELINE configs[3])",
         "ms_per_registration": ms, "registrations_per_s": 1e3 / ms, "iterations": r["iterations"],
         "derivative_passes": r["evaluations"], "n_voxels": r["n_voxels"],
         "translation_error_m": float(np.linalg.norm(r["T"][:3, 3] - T_gt[:3, 3])) if r["T"] is not None else None}
    fl = pmc.get("k_ndt_derivs", {}).get("f64_flops_per_source_point")
    roof = {"bound": "f64-valu", "kernel": "wm::k_ndt_derivs (score + gradient + Hessian passes, averaged)",
            "peak": F64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "avg_launch_us": us, "launches_timed": ev,
            "flops_per_source_point": fl, "flops_source": pmc.get("tag")}
    if fl and us > 0:
        roof["achieved"] = fl * n / (us * 1e-6) / 1e12
        roof["frac"] = roof["achieved"] / F64_VALU_PEAK_TFLOPS
    roof.update(counter_traffic(pmc, "k_ndt_derivs", us, copy_peak))
    e["roofline"] = roof
    try:
        e["in_flight"] = two_in_flight(torch, capi, ndt)
    except Exception as ex:
        e["in_flight"] = {"error": str(ex)}
    if with_cpu:
        from oracle import oracle_py as O
        m = 100_000
        rs, ts_, _ = synth.pair(m, seed=42, pattern="rings")
        t0 = time.perf_counter()
        O.ndt_align(rs, ts_, res=0.5)
        e["cpu_baseline"] = {"seconds_per_registration": time.perf_counter() - t0, "cores": 1, "kind": "port",
                             "sample": "the oracle's NDT on a %d<->%d pair of the same scene" % (m, m)}
    out.append(e)
    del d_ref, d_tgt

    # ---- configs[0]: the reference's own size, registered the MultiMatcher way -- a queue of pairs.
    # One launch takes 256 pairs (one compute unit each, target cloud in LDS: csrc/wm_small.hip);
    # every item is match() + estimateInfo() of the reference's worker loop.
    n, B = 10_000, 256
    base = [synth.pair(n, seed=100 + k, mode="resample")[:2] for k in range(8)]
    host_pairs = [base[k % 8] for k in range(B)]
    dev_clouds = [(torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)) for r, t in base]
    dev_pairs = [dev_clouds[k % 8] for k in range(B)]
    ms_h, got = median_ms(lambda: ctx.icp_batch_match(host_pairs, with_info=True, max_corr=3.0, max_iter=100), reps=5)
    ms_d, got = median_ms(lambda: ctx.icp_batch_match(dev_pairs, with_info=True, max_corr=3.0, max_iter=100), reps=5)
    ctx.set_source(base[0][0])
    ctx.set_target(base[0][1])
    ms_one, one = median_ms(lambda: ctx.icp_match(base[0][0], base[0][1], res=-1.0, max_corr=3.0, max_iter=100, carry_state=0))
    e = {"config": "ICPMatcher 10k<->10k (BASELINE configs[0]), %d queued pairs per launch (8 distinct pairs, each 32 times): "
                   "match() + estimateInfo() each, PCL's default stopping rules" % B,
         "pairs_per_launch": B,
         "registrations_per_s": B / (ms_h * 1e-3), "ms_per_batch": ms_h,
         "registrations_per_s_device_resident_clouds": B / (ms_d * 1e-3),
         "kernel_ms_per_batch": got[0]["align_ms"], "iterations_first_items": [g["iterations"] for g in got[:8]],
         "all_converged": all(g["rc"] == 0 for g in got),
         "one_pair_at_a_time_ms": ms_one, "one_pair_iterations": one["iterations"],
         "note": "host clouds: 2 x 160 kB per pair cross PCIe inside the timed call (one worker thread; "
                 "libwave_amd/host/bench_multimatcher runs the C++ wave::MultiMatcher pool on top of this)"}
    if with_cpu:
        from oracle import oracle_py as O
        t0 = time.perf_counter()
        m = O.IcpMatch(base[0][0], base[0][1], res=-1.0, multiscale_steps=0, incremental_float=0)
        m.lumold(3.0)
        e["cpu_baseline"] = {"seconds_per_registration": time.perf_counter() - t0, "cores": 1, "kind": "port",
                             "sample": "the oracle's match() + estimateLUMold on one of the pairs"}
        # ... and the reference's own way to throughput on the host: one registration per thread, all usable cores
        nthr = usable_cpus()
        if nthr > 1:
            per_thread = 4

            def cpu_worker(k):
                for j in range(per_thread):
                    r_, t_ = base[(k + j) % 8]
                    O.IcpMatch(r_, t_, res=-1.0, multiscale_steps=0, incremental_float=0).lumold(3.0)
            t0 = time.perf_counter()
            th = [threading.Thread(target=cpu_worker, args=(k,)) for k in range(nthr)]
            [t.start() for t in th]
            [t.join() for t in th]
            wall = time.perf_counter() - t0
            e["cpu_baseline"]["all_cores"] = {"registrations_per_s": nthr * per_thread / wall, "cores": nthr,
                                              "pattern": "MultiMatcher: %d threads, %d pairs each" % (nthr, per_thread)}
    out.append(e)
    del dev_clouds, dev_pairs

    # ---- the reference's DEFAULT matcher parameters (voxel filter 0.1 m + three coarser scales,
    # icp.hpp:54,59 -> icp.cpp:77-104) on scan-sized pairs, again a queue of them: all clouds of a call
    # go through pcl::VoxelGrid at once (cloud number above the leaf index in one sort key), then one
    # resident registration per pair and scale
    n, B = 55_000, 128
    base = [synth.pair(n, seed=200 + k, mode="resample")[:2] for k in range(4)]
    host_pairs = [base[k % 4] for k in range(B)]
    kw = dict(with_info=True, res=0.1, multiscale_steps=3, max_corr=3.0, max_iter=100)
    ms_h, got = median_ms(lambda: ctx.icp_batch_match(host_pairs, **kw), reps=3)
    ms_one, one = median_ms(lambda: ctx.icp_match(base[0][0], base[0][1], res=0.1, multiscale_steps=3, max_corr=3.0,
                                                  max_iter=100, carry_state=0))
    e = {"config": "ICPMatcher with its default parameters (res 0.1, multiscale_steps 3) on 55k<->55k pairs, %d queued pairs "
                   "per call: match() + estimateInfo() each" % B,
         "pairs_per_call": B, "registrations_per_s": B / (ms_h * 1e-3), "ms_per_batch": ms_h,
         "all_converged": all(g["rc"] == 0 for g in got), "one_pair_at_a_time_ms": ms_one,
         "finest_scale_points": got[0]["n_corr"],
         "note": "host clouds (2 x 0.9 MB per pair cross PCIe inside the timed call), one worker thread"}
    if with_cpu:
        from oracle import oracle_py as O
        t0 = time.perf_counter()
        m = O.IcpMatch(base[0][0], base[0][1], res=0.1, multiscale_steps=3, incremental_float=0)
        m.lumold(3.0)
        e["cpu_baseline"] = {"seconds_per_registration": time.perf_counter() - t0, "cores": 1, "kind": "port",
                             "sample": "the oracle's match() (4 scales) + estimateLUMold on one of the pairs"}
    out.append(e)

    # ---- GICPMatcher pairs the MultiMatcher way: a queue of them, 256 per launch, one compute unit each with the
    # whole of align inside the kernel (csrc/wm_gicp_small.hip); full-resolution 20k-point clouds
    # (256 DISTINCT pairs: a launch lasts as long as its slowest pair, so repeating a handful of pairs would
    # understate the spread of their durations)
    n, B = 20_000, 256
    base = [synth.pair(n, seed=300 + k, mode="resample")[:2] for k in range(B)]
    host_pairs = base
    dev_clouds = [(torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)) for r, t in base]
    dev_pairs = dev_clouds
    # the default objective (PCL's per-pair sums: every evaluation streams 104 bytes per pair of points, HBM-bound) ...
    ms_h, got = median_ms(lambda: ctx.gicp_batch_match(host_pairs), reps=2)
    ms_d, got = median_ms(lambda: ctx.gicp_batch_match(dev_pairs), reps=2)
    ms_one, one = median_ms(lambda: ctx.gicp_match(base[0][0], base[0][1]))
    ev_bytes = float(sum(g["evaluations"] for g in got) * n * 104)
    # ... and the opt-in statistics objective (a pair's 74 sums formed in the correspondence phase, nothing streamed per evaluation)
    STAT = capi.WM_GICP_OBJECTIVE_STATISTICS
    ms_hs, got_s = median_ms(lambda: ctx.gicp_batch_match(host_pairs, objective=STAT), reps=3)
    ms_ds, got_s = median_ms(lambda: ctx.gicp_batch_match(dev_pairs, objective=STAT), reps=3)
    stat_entry = {"registrations_per_s": B / (ms_hs * 1e-3), "registrations_per_s_device_resident_clouds": B / (ms_ds * 1e-3),
                  "kernel_ms_per_batch": got_s[0]["kernel_ms"], "all_converged": all(g["rc"] == 0 for g in got_s),
                  "outer_iterations_first_items": [g["iterations"] for g in got_s[:8]],
                  "objective_evaluations_first_items": [g["evaluations"] for g in got_s[:8]],
                  "objective": "OPT-IN (WM_GICP_OBJECTIVE_STATISTICS), not the reference's arithmetic: a pair's 74 sums are formed in the "
                               "correspondence phase, wave 0's optimiser evaluates them as scalar work"}
    e = {"config": "GICPMatcher 20k<->20k, %d distinct queued pairs per launch (k = 10 covariances, PCL's default stopping rules)" % B,
         "pairs_per_launch": B, "registrations_per_s": B / (ms_h * 1e-3), "ms_per_batch": ms_h,
         "registrations_per_s_device_resident_clouds": B / (ms_d * 1e-3), "kernel_ms_per_batch": got[0]["kernel_ms"],
         "outer_iterations_first_items": [g["iterations"] for g in got[:8]],
         "objective_evaluations_first_items": [g["evaluations"] for g in got[:8]],
         "all_converged": all(g["rc"] == 0 for g in got),
         "one_pair_at_a_time_ms": ms_one,
         "first_item_equals_the_one_pair_path_bit_for_bit": bool(np.array_equal(got[0]["T"], one["T"])) and got[0]["evaluations"] == one["evaluations"],
         "objective": "PCL's per-pair sums (the default = the reference's algorithm)",
         "roofline": {"bound": "hbm", "kernel": "wm::k_gicp_small<10>, per-pair objective: the evaluations stream 104 bytes per pair of points",
                      "algorithmic_bytes_per_launch": ev_bytes, "achieved": ev_bytes / (got[0]["kernel_ms"] * 1e-3) / 1e9,
                      "peak": 8000.0, "unit": "GB/s", "frac": ev_bytes / (got[0]["kernel_ms"] * 1e-3) / 1e9 / 8000.0,
                      "note": "whole-kernel time (grids, covariances, searches included) against the evaluations' bytes alone"},
         "statistics": stat_entry,
         "note": "host clouds: 2 x 320 kB per pair cross PCIe inside the timed call (one worker thread; "
                 "libwave_amd/host/bench_multimatcher with BENCH_MATCHER=gicp runs the C++ wave::MultiMatcher pool on top of this)"}
    out.append(e)

    # ---- NDTMatcher pairs the same way: voxel model + align inside one workgroup per pair (csrc/wm_ndt_small.hip);
    # the same 20k-point clouds, 1 m voxels
    ms_h, got = median_ms(lambda: ctx.ndt_batch_match(host_pairs, res=1.0), reps=3)
    ms_d, got = median_ms(lambda: ctx.ndt_batch_match(dev_pairs, res=1.0), reps=3)

    def ndt_one():
        ctx.set_source(base[0][0])
        ctx.set_target(base[0][1])
        return ctx.ndt_align(res=1.0)
    ms_one, one = median_ms(ndt_one)
    e = {"config": "NDTMatcher 20k<->20k, 1 m voxels, %d distinct queued pairs per launch (More-Thuente line search, PCL's defaults)" % B,
         "pairs_per_launch": B, "registrations_per_s": B / (ms_h * 1e-3), "ms_per_batch": ms_h,
         "registrations_per_s_device_resident_clouds": B / (ms_d * 1e-3), "kernel_ms_per_batch": got[0]["kernel_ms"],
         "iterations_first_items": [g["iterations"] for g in got[:8]],
         "derivative_passes_first_items": [g["evaluations"] for g in got[:8]],
         "all_converged": all(g["rc"] == 0 for g in got),
         "one_pair_at_a_time_ms": ms_one,
         "first_item_vs_the_one_pair_path_max_abs_dT": float(np.abs(got[0]["T"] - one["T"]).max()),
         "note": "a launch lasts as long as its slowest pair (30 to 140 passes on these pairs); the C++ pool keeps several launches in "
                 "flight (libwave_amd/host/bench_multimatcher with BENCH_MATCHER=ndt)"}
    out.append(e)
    del dev_clouds, dev_pairs
    ctx.close()
    prof.close()
    return out


def in_flight_throughput(torch, capi, d_ref, d_tgt, h_ref, h_tgt, a, crews=(1, 2, 4), regs_per_worker=24):
    """BASELINE configs[1] the way the reference gets THROUGHPUT: wave::MultiMatcher's pattern (multi_matcher.hpp:32,
    impl/multi_matcher_impl.hpp:30-64) -- one matcher per worker thread, every worker registering its own pairs --
    with 1M<->1M pairs at full resolution and 50 forced iterations.  Here a worker is a host thread with its own
    wm_ctx (own HIP stream, own device buffers); the registrations of different workers overlap on the one GPU: one
    worker's single-workgroup tails and cloud preparation run under another's searches.  Clouds: device-resident
    (as `value`) and pinned host memory (H2D inside the step).  ctypes releases the GIL inside the C-ABI calls."""
    out = []
    for mode, (r_, t_) in (("device-resident clouds", (d_ref, d_tgt)), ("pinned host clouds (H2D inside)", (h_ref, h_tgt))):
        rows = []
        for crew in crews:
            ctxs = [capi.Context(0) for _ in range(crew)]

            def reg(c):
                c.set_source(r_)
                c.set_target(t_)
                return c.icp_align(max_corr=a.max_corr, force_iterations=a.iters, nn_method=capi.WM_NN_GRID, profile=0,
                                   carry_state=0)
            for c in ctxs:  # warm-up: allocations, the tuned cell size
                reg(c)
                reg(c)
            torch.cuda.synchronize()
            errs = []
            start = threading.Barrier(crew + 1)

            def worker(c):
                start.wait()
                for _ in range(regs_per_worker):
                    r = reg(c)
                    if r["rc"] != 0:
                        errs.append(r["rc"])
            th = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
            [t.start() for t in th]
            start.wait()
            t0 = time.perf_counter()
            [t.join() for t in th]
            wall = time.perf_counter() - t0
            for c in ctxs:
                c.close()
            rows.append({"workers": crew, "registrations": crew * regs_per_worker, "seconds": wall,
                         "registrations_per_s": crew * regs_per_worker / wall, "failed": len(errs)})
        out.append({"clouds": mode, "rows": rows,
                    "speedup_2_in_flight": rows[1]["registrations_per_s"] / rows[0]["registrations_per_s"] if len(rows) > 1 else None})
    return out


def two_in_flight(torch, capi, reg, regs_per_worker=16):
    """registrations/s of `reg(ctx)` with one and with two worker threads, each with its own context (the MultiMatcher
    pattern on one GPU, as in_flight_throughput): what the host round trips of a GICP / NDT registration leave idle."""
    rows = {}
    for crew in (1, 2):
        ctxs = [capi.Context(0) for _ in range(crew)]
        for c in ctxs:
            reg(c)
            reg(c)
        torch.cuda.synchronize()
        start = threading.Barrier(crew + 1)

        def worker(c):
            start.wait()
            for _ in range(regs_per_worker):
                reg(c)
        th = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
        [t.start() for t in th]
        start.wait()
        t0 = time.perf_counter()
        [t.join() for t in th]
        rows[crew] = crew * regs_per_worker / (time.perf_counter() - t0)
        for c in ctxs:
            c.close()
    return {"registrations_per_s_1_in_flight": rows[1], "registrations_per_s_2_in_flight": rows[2],
            "speedup_2_in_flight": rows[2] / rows[1]}


def assemble_line(a, world, r, T_gt, elapsed, step_ms, nn_ms, nn_launches, cert_ms, cert_launches, parallelism,
                  pmc=None, peak_copy=None, sharded=False, ar_us=None):
    """The bench line of rank 0 from one run's measurements -- `r`: the last timed step's result dict (capi's
    icp_align / icp_align_sharded), the event-timed search totals, the wall time of the `a.steps` timed steps.  A function
    of its own so that the N > 1 line (config.sharding from the sharded result's keys) is exercised without GPUs
    (tests/test_bench_helpers_cpu.py): the first real multi-GPU run must not end in a KeyError."""
    pmc = pmc or {}
    n_total = a.points * world
    T = r["T"]
    err_t = float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))
    # whole-job throughput in 1M-point registration equivalents (weak scaling: the
    # N-GPU job registers an N x 1M-point pair, i.e. N units of the metric's size)
    regs_per_s_raw = a.steps / elapsed
    value = regs_per_s_raw * (n_total / 1_000_000.0)
    nn_us = nn_ms / max(nn_launches, 1) * 1e3
    pts_per_launch = a.points  # queries handled by one rank's launch
    alg_bytes = 32.0 * pts_per_launch  # 12N + 12M + 8N with N = M
    achieved = alg_bytes / (nn_us * 1e-6) / 1e9 if nn_us > 0 else 0.0
    out = {
        "metric": "point-cloud registrations/sec (1M<->1M pts, ICP)",
        "value": value, "unit": "registrations/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": "ICPMatcher %d<->%d synthetic XYZ clouds (BASELINE configs[%d]), DEVICE-RESIDENT "
                        "(both clouds in HBM before the timed region), %d forced iterations, max_corr=%g, "
                        "res=-1; step = set_source + set_target (index build) + align" % (
                            n_total, n_total, 1 if world == 1 else 4, a.iters, a.max_corr),
            "arithmetic": "f32 points and distances, f64 reductions and solve",
            "scene": "base scene x%d tiled along x at constant density; T_gt rotation / %d" % (world, world),
            "points_per_cloud_total": n_total, "points_per_gpu": a.points,
            "iterations": a.iters, "parallelism": parallelism,
            "registrations_per_s_raw": regs_per_s_raw,
            "icp_iterations_per_s": regs_per_s_raw * a.iters,
            "final_translation_error_m": err_t, "grid_cell_m": r.get("grid_cell"),
            "cert_launches_per_registration": r.get("cert_launches"),
            "ms_each_step_rank0": [round(t, 3) for t in step_ms],
        },
        "roofline": None,
    }
    # The correspondence step of an iteration is ONE launch of one of two kernels: the full search
    # (k_nn_grid) while the clouds still move, the certificate kernel (k_nn_cert: previous match proved
    # still nearest, search only where the proof fails) once a step is small.  Both leave the same keys
    # and carry the iteration's statistics; SURVEY 8(d)'s 32 B x n is the algorithmic traffic of either.
    grid_launches = nn_launches - cert_launches
    kernels = []
    for name, key, ms, launches in (("wm::k_nn_grid", "k_nn_grid", nn_ms - cert_ms, grid_launches),
                                    ("wm::k_nn_cert", "k_nn_cert", cert_ms, cert_launches)):
        if launches <= 0:
            continue
        us = ms / launches * 1e3
        # coalesced streams of a launch: source points + previous keys + previous matches (k_nn_grid),
        # source points + matches + positions-and-bounds (k_nn_cert); everything else it reads is gathered
        streams = (16.0 + 8.0 + 16.0 if key == "k_nn_grid" else 48.0) * pts_per_launch
        tr = pmc_traffic_bytes(pmc, key, streams) if world == 1 else None
        tr_upper = pmc_traffic_bytes(pmc, key) if world == 1 else None
        # the roof that BINDS, next to the one north_star names: vector-ALU issue.  A SIMD issues one wave64 VALU
        # instruction per 4 cycles: 256 CUs x 4 SIMDs x 2.4 GHz / 4 = 614.4 G wave-instructions/s; achieved = the
        # kernel's SQ_INSTS_VALU per launch (committed --pmc pass of this command, stamped with the kernel sources)
        # over this run's event-timed launch duration.  (A kernel also waits on its gathers: 1.0 is not reachable
        # for a search; the fraction says how much of the launch the vector ALUs were the busy unit.)
        valu = (pmc.get(key) or {}).get("SQ_INSTS_VALU_per_dispatch") if world == 1 else None
        valu_block = None
        if valu and us > 0:
            valu_block = {"bound": "valu-issue", "achieved": valu / (us * 1e-6) / 1e9, "peak": VALU_ISSUE_PEAK_GINST,
                          "unit": "G wave64-instructions/s", "frac": valu / (us * 1e-6) / 1e9 / VALU_ISSUE_PEAK_GINST,
                          "wave_instructions_per_launch": valu,
                          "wave_instructions_per_64_queries": valu / (pts_per_launch / 64.0)}
        kernels.append({"name": name, "launches_timed": launches, "avg_launch_us": us,
                        "share_of_search_time": ms / nn_ms if nn_ms > 0 else None,
                        "achieved": alg_bytes / (us * 1e-6) / 1e9, "frac": alg_bytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                        "traffic": tr, "traffic_if_all_streamed_x2": tr_upper,
                        "hbm_util": (tr / (us * 1e-6) / 1e9 / peak_copy) if (tr and peak_copy) else None,
                        "valu_issue": valu_block})
        if valu_block:
            out["config"]["valu_issue_frac_%s" % key] = valu_block["frac"]
    traffic = None
    if kernels and all(k["traffic"] for k in kernels):
        traffic = sum(k["traffic"] * k["launches_timed"] for k in kernels) / max(nn_launches, 1)
    out["roofline"] = {
        "bound": "hbm",
        "kernel": "the correspondence step of an ICP iteration: one launch of wm::k_nn_grid or wm::k_nn_cert "
                  "(search + the iteration's statistics); launch-weighted over both, per kernel in `kernels`",
        "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": traffic,
        "hbm_util": (traffic / (nn_us * 1e-6) / 1e9 / peak_copy) if (traffic and peak_copy) else None,
        "traffic_source": ("profiles/pmc_latest.json, tag %s (separate rocprofv3 --pmc passes of this "
                           "command; a committed measurement, not this run's; its csrc_sha256 stamp matches "
                           "the kernels in the tree); FETCH_SIZE calibrated on this part: coalesced streams are "
                           "tallied at half their bytes, gathers at what they move (profiles/r04_fetch_size_calibration.json)"
                           % pmc.get("tag")) if pmc.get("tag") else pmc.get("stale"),
        "peak_measured_copy": peak_copy,
        "peak_measured_copy_method": "float4 grid-stride copy kernel, 1 GiB in + 1 GiB out, 10 launches (wm_debug_copy_bandwidth)",
        "algorithmic_bytes_per_launch": alg_bytes,
        "avg_launch_us": nn_us, "launches_timed": nn_launches, "kernels": kernels,
        # launch-weighted over both kernels: the binding roof (see `kernels[*].valu_issue`)
        "valu_issue": ({"bound": "valu-issue", "peak": VALU_ISSUE_PEAK_GINST, "unit": "G wave64-instructions/s",
                        "achieved": sum(k["valu_issue"]["wave_instructions_per_launch"] * k["launches_timed"] for k in kernels)
                                    / (nn_ms * 1e-3) / 1e9,
                        "frac": sum(k["valu_issue"]["wave_instructions_per_launch"] * k["launches_timed"] for k in kernels)
                                / (nn_ms * 1e-3) / 1e9 / VALU_ISSUE_PEAK_GINST}
                       if kernels and nn_ms > 0 and all(k["valu_issue"] for k in kernels) else None),
        "note": "an exact gather search: what binds is the vector ALU and the L1 address path of the candidate "
                "walk (k_nn_grid) and instruction issue + workgroup dispatch (k_nn_cert), not HBM (DESIGN.md "
                "sections 4.1 / 5)",
    }
    if sharded:
        # where rank 0's time went in the last (event-bracketed) step, and what an all-reduce costs alone
        out["config"]["sharding"] = {
            k: r.get(k) for k in ("plan_ms", "compact_ms", "index_ms", "iter_ms", "allreduce_ms", "n_tgt_local",
                                  "n_src_local", "rccl_ranks", "shard_attempts", "owned_violations", "align_ms",
                                  "exchange_in_kernel")}
        out["config"]["sharding"]["allreduce_us_isolated"] = ar_us
        out["config"]["sharding"]["exchange"] = (
            "mailboxes: every rank's 34-double block stored into every peer's mailbox over xGMI and summed in rank "
            "order INSIDE the solve kernel (wm_xchg.hpp)" if r.get("exchange_in_kernel") else
            "ncclAllReduce(34 f64) on the context's stream between a rank's sums and its solve")
        out["config"]["sharding"]["note"] = (
            "rank 0, last timed step: plan/compact = device time of slab planning and band selection; index = host "
            "wall time of enqueueing the local clouds' order and grid; iter = host wall time of the 50 iterations; "
            "allreduce = sum of the 50 ncclAllReduce by HIP events (0 when the exchange runs inside the solve kernel); "
            "isolated = one exchange alone, back to back (a kernel of its own there)")
    return out


def relaunch(n):
    """`python bench.py --gpus N` without a launcher: exec `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <same arguments>`."""
    import socket
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    argv = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
            "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    sys.stderr.flush()
    os.execv(sys.executable, argv)


def main():
    a = parse()
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        if world == 1 and a.gpus > 1 and "RANK" not in os.environ:
            # launched plainly (`python bench.py --gpus N`): become the launcher -- one process per GPU under
            # torch.distributed.run, exactly the line the driver uses, rendezvous on 127.0.0.1
            relaunch(a.gpus)
        a.gpus = world
    if os.environ.get("WM_BENCH_DRY_LAUNCH") == "1":
        # launch-line check (tests/test_bench_launch_cpu.py, no GPU needed): the ranks exist, find each other
        # and agree on the world -- everything up to the communicator's set-up -- and stop there
        t = torch.tensor([rank], dtype=torch.int64)
        if "RANK" in os.environ:
            import torch.distributed as dist
            dist.init_process_group("gloo")
            dist.all_reduce(t)
            dist.destroy_process_group()
        print("dry-launch rank %d of %d: ranks sum %d" % (rank, world, int(t.item())), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback exists)")
    if torch.cuda.device_count() < world and "LOCAL_RANK" in os.environ and local_rank >= torch.cuda.device_count():
        raise SystemExit("--gpus %d: this node shows %d HIP devices" % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dist = None
    force_sharded = os.environ.get("WM_BENCH_FORCE_SHARDED") == "1"  # plumbing check at N=1
    if force_sharded:
        os.environ["WM_SHARD_FORCE"] = "1"
    if world > 1 or (force_sharded and "RANK" in os.environ):
        # (a one-rank group under torch.distributed.run still sends every iteration's block
        # through RCCL: the whole N > 1 code path on a single GPU)
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import __graft_entry__ as g
    if rank == 0:
        g.build()
    if dist:
        dist.barrier()
    from libwave_amd import capi, synth

    n_total = a.points * world
    # weak scaling: `world` tiles of the base scene side by side (same density, longer map);
    # world == 1 is the plain 1M<->1M pair of BASELINE configs[1]
    ref, tgt, T_gt = synth.pair_tiled(a.points, world, seed=42)
    dev = torch.device("cuda", local_rank)
    d_ref = torch.from_numpy(ref).to(dev)
    d_tgt = torch.from_numpy(tgt).to(dev)
    ctx = capi.Context(local_rank)
    comm = None
    torch.cuda.synchronize()

    exchange_fallback = False
    if dist is None:
        def step(profile, r_=d_ref, t_=d_tgt):
            ctx.set_source(r_)
            ctx.set_target(t_)
            return ctx.icp_align(max_corr=a.max_corr, force_iterations=a.iters,
                                 nn_method=capi.WM_NN_GRID, profile=profile, carry_state=0)
        parallelism = "single"
    else:
        def make_comm():
            # the RCCL id: made by rank 0, handed to every rank (the one thing torch.distributed carries)
            uid = [capi.Comm.unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            return capi.Comm.init_rank(local_rank, uid[0], rank, world)

        def all_ranks_ok(ok):
            t = torch.tensor([1 if ok else 0], device=dev, dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return bool(int(t.item()))
        box = {"ctx": ctx, "comm": make_comm()}

        def one(profile):
            return box["ctx"].icp_align_sharded(box["comm"], d_ref, d_tgt, max_corr=a.max_corr, force_iterations=a.iters,
                                                nn_method=capi.WM_NN_GRID, profile=profile, carry_state=0)

        def rebuild_collective():
            # (the exchange through the ranks' mailboxes has never run over xGMI in the builder's container: if the
            # very first registration fails on ANY rank, every rank drops its communicator and context and starts
            # over with the collective exchange -- ncclAllReduce between a rank's sums and its solve)
            os.environ["WM_COMM_P2P"] = "0"
            for k in ("comm", "ctx"):
                try:
                    box[k].close()
                except Exception:
                    pass
            box["ctx"] = capi.Context(local_rank)
            box["comm"] = make_comm()
        exchange_fallback = first_step_with_fallback(lambda: one(1), rebuild_collective, all_ranks_ok, capi.WmError)
        ctx, comm = box["ctx"], box["comm"]

        def step(profile):
            return one(profile)
        parallelism = ("target x-slabs x%d + one exchange of 34 f64 per iteration inside the library (mailboxes over "
                       "xGMI inside the solve kernel; ncclAllReduce where they cannot be set up)" % world)

    # (no collector pauses inside the timed region: a capture of this command showed a lone 7 ms step among 3.75 ms
    # ones, profiles/r05m_bench_line_noprof.json; the interpreter's collector is the one pause this script can rule
    # out.  Collected BEFORE the warm-up: a collection between warm-up and timing leaves the GPU idle for tens of
    # milliseconds and the first timed step 0.3 ms slower, gpurun_out/r05n_jitter)
    # (--full: the device's copy rate -- what `roofline.hbm_util` is a fraction of -- is measured BEFORE the registrations:
    # it is the bench's one other device-wide measurement, and a device that has just moved 40 GB enters the warm-up at
    # its working clocks rather than from idle)
    peak_copy_early = ctx.copy_bandwidth() if (a.full and world == 1 and rank == 0) else None
    import gc
    gc.collect()
    gc.disable()
    for _ in range(a.warmup):
        r = step(1)
    torch.cuda.synchronize()
    ar_us = ctx.allreduce_probe(comm) if (a.full and comm is not None) else None
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    nn_ms = 0.0
    nn_launches = 0
    cert_ms = 0.0
    cert_launches = 0
    step_ms = []
    for k in range(a.steps):
        # HIP events around every launch of the correspondence kernel cost a barrier packet
        # each (~0.35 ms per registration), so they bracket the launches of ONE step per twenty
        # (at least the last: 50 launches, every iteration of one registration -- each step runs
        # the same 50); the others run exactly as a caller's registration would
        timed = (k % 20 == 19) or k == a.steps - 1
        t_step = time.perf_counter()
        r = step(1 if timed else 0)
        step_ms.append((time.perf_counter() - t_step) * 1e3)  # (align blocks: host time = step time)
        if timed:
            nn_ms += r["nn_ms"]
            nn_launches += r["nn_launches"]
            cert_ms += r.get("nn_cert_ms", 0.0)
            cert_launches += r.get("cert_launches", 0)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    if dist:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if a.dump_outputs and rank == 0:
        # (before anything else runs on the context: the correspondences are the last timed step's)
        dump_outputs(a.dump_outputs, r, ctx if dist is None else None)

    # N > 1 (or the one-rank plumbing check), --full: north_star names "RCCL all-reduce over xGMI" as the exchange, the
    # library's default is its own mailbox exchange inside the solve kernel.  When mailboxes ran, the SAME registration is
    # timed once more, shortly, with the group rebuilt on ncclAllReduce (WM_COMM_P2P=0): the line carries both.
    other_exchange = None
    if (a.full and comm is not None and not exchange_fallback and bool(r.get("exchange_in_kernel"))
            and os.environ.get("WM_COMM_P2P", "1") != "0"):
        try:
            rebuild_collective()
            ctx, comm = box["ctx"], box["comm"]
            for _ in range(2):
                one(0)
            torch.cuda.synchronize()
            dist.barrier()
            t1 = time.perf_counter()
            k2 = max(3, min(a.steps, 5))
            for _ in range(k2):
                r2 = one(0)
            torch.cuda.synchronize()
            dist.barrier()
            tt = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            other_exchange = {"exchange": "ncclAllReduce(34 f64) on the context's stream between a rank's sums and its solve",
                              "steps": k2, "ms_per_step": float(tt.item()) / k2 * 1e3,
                              "exchange_in_kernel": int(r2.get("exchange_in_kernel", 0)),
                              "same_transform_as_the_mailbox_run": bool(np.array_equal(r2["T"], r["T"]))}
        except Exception as ex:  # (never lose the line over the extra measurement)
            other_exchange = {"error": str(ex)}

    if rank == 0:
        pmc = pmc_summary() if world == 1 else {}
        peak_copy = peak_copy_early if world == 1 else None
        out = assemble_line(a, world, r, T_gt, elapsed, step_ms, nn_ms, nn_launches, cert_ms, cert_launches, parallelism,
                            pmc=pmc, peak_copy=peak_copy, sharded=comm is not None, ar_us=ar_us)
        if comm is not None:
            out["config"]["sharding"]["exchange_fell_back_to_collective"] = bool(exchange_fallback)
            out["config"]["sharding"]["exchange_that_ran"] = "mailboxes" if r.get("exchange_in_kernel") else "ncclAllReduce"
            out["config"]["sharding"]["ms_per_step_this_exchange"] = elapsed / a.steps * 1e3
            if other_exchange is not None:
                out["config"]["sharding"]["collective_exchange"] = other_exchange
                if "ms_per_step" in other_exchange:
                    # (scalar keys of `config`: the driver's record keeps those)
                    out["config"]["ms_per_step_mailbox_exchange"] = elapsed / a.steps * 1e3
                    out["config"]["ms_per_step_rccl_allreduce_exchange"] = other_exchange["ms_per_step"]
        value = out["value"]
        if a.full and world == 1 and dist is None and not a.no_host_clouds:
            # the same registration from HOST clouds: H2D of both clouds inside the step
            hc = {}
            for name, (hr, ht) in (("pageable", (ref, tgt)),
                                   ("pinned", (torch.from_numpy(ref).pin_memory().numpy(),
                                               torch.from_numpy(tgt).pin_memory().numpy()))):
                for _ in range(2):
                    step(0, hr, ht)
                ts = []
                for _ in range(max(3, min(a.steps, 6))):
                    t1 = time.perf_counter()
                    step(0, hr, ht)
                    ts.append((time.perf_counter() - t1) * 1e3)
                hc[name] = {"ms_per_registration": float(np.median(ts)), "registrations_per_s": 1e3 / float(np.median(ts))}
            hc["note"] = "wm_set_source / wm_set_target with WM_MEM_HOST: 2 x 16 MB cross PCIe inside the step"
            out["config"]["host_clouds"] = hc
            # SURVEY 8(d) / BASELINE.md section 3 define a registration as INCLUDING the upload of both clouds.  Scalar
            # keys of `config` (the driver's record keeps those; it drops nested objects and extra top-level keys):
            out["config"]["registrations_per_s_h2d_inclusive"] = hc["pinned"]["registrations_per_s"]
            out["config"]["ms_per_registration_h2d_inclusive"] = hc["pinned"]["ms_per_registration"]
            out["config"]["registrations_per_s_h2d_inclusive_pageable"] = hc["pageable"]["registrations_per_s"]
            out["config"]["ms_per_registration_device_resident"] = elapsed / a.steps * 1e3
            # SURVEY 8(d) counts the upload of both clouds as part of a registration: that rate, first class
            out["value_h2d_inclusive"] = hc["pinned"]["registrations_per_s"]
            out["value_h2d_inclusive_note"] = ("the same registration from pinned HOST clouds (both uploads inside the "
                                               "timed step); `value` is with the clouds already in HBM")
        if a.full and world == 1 and dist is None and not a.no_in_flight:
            # configs[1] with MORE THAN ONE registration in flight (the headline `value` stays one at a time)
            try:
                pin_r, pin_t = torch.from_numpy(ref).pin_memory().numpy(), torch.from_numpy(tgt).pin_memory().numpy()
                fl = in_flight_throughput(torch, capi, d_ref, d_tgt, pin_r, pin_t, a)
                out["in_flight"] = {"config": "ICPMatcher 1M<->1M, %d forced iterations (BASELINE configs[1]), the MultiMatcher "
                                              "pattern: one matcher (wm_ctx + stream) per worker thread on ONE GPU" % a.iters,
                                    "results": fl}
                for blk, suffix in ((fl[0], ""), (fl[1], "_h2d_inclusive")):
                    for row in blk["rows"]:
                        out["config"]["registrations_per_s_%d_in_flight%s" % (row["workers"], suffix)] = row["registrations_per_s"]
            except Exception as ex:  # (never lose the line over the extra measurement)
                out["in_flight"] = {"error": str(ex)}
        if a.full and world == 1 and not a.no_other_configs:
            out["other_configs"] = other_configs(torch, dev, capi, synth, pmc, not a.no_cpu_baseline, peak_copy)
        if a.full and world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(ref, tgt, a.iters, a.max_corr, a.cpu_iters)
            out["config"]["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
            if "all_cores" in out["cpu_baseline"]:
                out["config"]["speedup_vs_cpu_all_cores"] = value / out["cpu_baseline"]["all_cores"]["value"]
        print(json.dumps(out))
    if comm is not None:
        comm.close()
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
