"""wm_outlier_filter timing: device milliseconds per call (wm_outlier_stats.kernel_ms: HIP events from the cloud's
packing to the kept list, the grid build and its two small fetches included) and host milliseconds per call (clock
around a call, which ends in its own synchronise), with the cloud resident in device memory, on synth.scene(1M) and the
64-ring synth.scene_rings(2M).  Statistical filter: mean_k 8 and 20, stddev_mult 1; radius filter: 0.2 m and 0.5 m,
min_neighbors 5, with counts_out (exact counts) and without (a search stops at min_neighbors).  Every figure is the
median of --calls calls after --warmup, with the fastest and slowest call beside it.  Prints one JSON line.

--cell-div D[,D...]  the radius filter again under option outlier_cell_div = D (the grid cell is max(automatic,
                     radius / D)): the cell rule's effect.
--yardstick N        N rounds of: the statistical filter at mean_k 9 (k_outlier_mean_dist<10>), then wm_gicp_covariances
                     at k = 10 with the same cloud as source and target (k_gicp_cov<10>, on the source's grid with
                     Morton-ordered queries and on the target's level-0 grid in grid order).  Meant to run under
                     `rocprofv3 --kernel-trace --stats`, whose per-kernel times are the comparison; nothing else is timed.
--batch S[,S...]     adds the key "batch": wm_outlier_filter_batch over S scans against the same S scans through
                     wm_outlier_filter one after the other on the same context, the two alternating; host ms PER SCAN
                     (clock around calls that end in their own synchronise), the median of --rounds rounds, one entry
                     per repeat (--repeats: their range is the run-to-run spread).  Device input; statistical mean_k 8
                     (stddev_mult 1) and radius 0.5 m (min_neighbors 5, no counts_out); the scans: 4 000 ... 20 000
                     points each, every 50th point of synth.scene(1M) and every 100th of synth.scene_rings(2M) from
                     offset k.  --skip-plain leaves the single-call part out; --loop-only times the loop of single
                     calls alone (what a library without the batch entry can run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, cloud, calls, warmup, **params):
    for _ in range(warmup):
        ctx.outlier_filter(cloud, **params)
    dev, host = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = ctx.outlier_filter(cloud, **params)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(r["kernel_ms"])
    return {"device_ms": round(float(np.median(dev)), 4), "device_ms_min_max": [round(float(min(dev)), 4), round(float(max(dev)), 4)],
            "host_ms": round(float(np.median(host)), 4), "kept": int(len(r["indices"])), "n_finite": int(r["n_finite"])}


def bench_batch(ctx, host_clouds, sizes, rounds, warmup, repeats, loop_only):
    import torch
    top = max(sizes)
    work = {}
    for name, (host, step) in host_clouds.items():
        work[name] = [torch.from_numpy(np.ascontiguousarray(host[k % step::step][:4000 + (k * 3000) % 16001])).to("cuda")
                      for k in range(top)]
    methods = {"statistical_k8": dict(method=0, mean_k=8, stddev_mult=1.0),
               "radius_0.5": dict(method=1, radius=0.5, min_neighbors=5, counts=False)}
    out = {"metric": "host ms per scan (median of rounds; one entry per repeat)", "rounds": rounds, "repeats": repeats}
    for name, scans in work.items():
        out[name] = {"points_per_scan": int(np.mean([len(s) for s in scans[:min(sizes)]]))}
    torch.cuda.synchronize()
    for _ in range(repeats):  # the whole measurement, again
        for name, scans in work.items():
            for mname, params in methods.items():
                for S_ in sizes:
                    clouds = scans[:S_]
                    for _ in range(max(warmup // S_, 3)):
                        for c in clouds:
                            ctx.outlier_filter(c, **params)
                        if not loop_only:
                            ctx.outlier_filter_batch(clouds, **params)
                    tl, tb = [], []
                    for _ in range(rounds):
                        t0 = time.perf_counter()
                        for c in clouds:
                            ctx.outlier_filter(c, **params)
                        t1 = time.perf_counter()
                        if not loop_only:
                            ctx.outlier_filter_batch(clouds, **params)
                        t2 = time.perf_counter()
                        tl.append((t1 - t0) * 1e3 / S_)
                        tb.append((t2 - t1) * 1e3 / S_)
                    cell = out[name].setdefault("%s_S%d" % (mname, S_), {"loop_ms_per_scan": [], "batch_ms_per_scan": []})
                    cell["loop_ms_per_scan"].append(round(float(np.median(tl)), 4))
                    if not loop_only:
                        cell["batch_ms_per_scan"].append(round(float(np.median(tb)), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="", help="S[,S...]: also time wm_outlier_filter_batch against a loop of single calls")
    ap.add_argument("--rounds", type=int, default=50, help="rounds of a --batch cell")
    ap.add_argument("--repeats", type=int, default=3, help="repeats of the whole --batch measurement")
    ap.add_argument("--skip-plain", action="store_true", help="with --batch: leave the single-call part out")
    ap.add_argument("--loop-only", action="store_true", help="with --batch: only the loop of single calls")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clouds", default="scene_1m,rings_2m")
    ap.add_argument("--cell-div", default="", help="D[,D...]: the radius filter under option outlier_cell_div = D")
    ap.add_argument("--yardstick", type=int, default=0, help="rounds of mean_k 9 + wm_gicp_covariances(k = 10), for a kernel trace")
    a = ap.parse_args()
    import torch
    from libwave_amd import capi, synth
    make = {"scene_1m": lambda: synth.scene(1_000_000, seed=42), "rings_2m": lambda: synth.scene_rings(2_000_000, seed=42)}
    ctx = capi.Context(0)
    out = {"metric": "wm_outlier_filter ms per call, cloud in device memory (median of calls)", "calls": a.calls}
    sizes = [int(x) for x in a.batch.split(",") if x]
    for name in [c for c in a.clouds.split(",") if c and not (sizes and a.skip_plain)]:
        host = make[name]()
        cloud = torch.from_numpy(host).to("cuda")
        torch.cuda.synchronize()
        row = {"points": int(len(host))}
        if a.yardstick:
            for _ in range(a.yardstick):
                ctx.outlier_filter(cloud, method=0, mean_k=9, stddev_mult=1.0)
                ctx.set_source(cloud)
                ctx.set_target(cloud)
                ctx.gicp_covariances(10, 1e-3)
            row["yardstick_rounds"] = a.yardstick
        else:
            for mean_k in (8, 20):
                row["statistical_k%d" % mean_k] = timed(ctx, cloud, a.calls, a.warmup, method=0, mean_k=mean_k, stddev_mult=1.0)
            for r in (0.2, 0.5):
                for counts in (True, False):
                    key = "radius_%g_%s" % (r, "counts" if counts else "stop_at_min")
                    row[key] = timed(ctx, cloud, a.calls, a.warmup, method=1, radius=r, min_neighbors=5, counts=counts)
            for div in [float(x) for x in a.cell_div.split(",") if x]:
                ctx.set_option("outlier_cell_div", div)
                for r in (0.2, 0.5):
                    for counts in (True, False):
                        key = "radius_%g_%s_div%g" % (r, "counts" if counts else "stop_at_min", div)
                        row[key] = timed(ctx, cloud, a.calls, a.warmup, method=1, radius=r, min_neighbors=5, counts=counts)
                ctx.set_option("outlier_cell_div", 2.0)
        out[name] = row
        del cloud
    if sizes:
        cut = {"scene_1m_cut": (make["scene_1m"](), 50), "rings_2m_cut": (make["rings_2m"](), 100)}
        out["batch"] = bench_batch(ctx, cut, sizes, a.rounds, a.warmup, a.repeats, a.loop_only)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
