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
                     `rocprofv3 --kernel-trace --stats`, whose per-kernel times are the comparison; nothing else is timed."""
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


def main():
    ap = argparse.ArgumentParser()
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
    for name in [c for c in a.clouds.split(",") if c]:
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
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
