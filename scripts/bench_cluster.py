"""wm_cluster_extract timing: device milliseconds per call (wm_cluster_stats.kernel_ms: HIP events from the cloud's
packing to the last output, the grid build, its small fetches and the fetch of the counters included) and host
milliseconds per call (clock around a call, which ends in its own synchronise), with the cloud resident in device
memory, on synth.scene(1M) and on the obstacle points wm_ground_segment keeps from the 64-ring synth.scene_rings(2M)
(filtered on the device: wm_ground_segment_batch with points_out in device memory), at tolerance 0.2 m and 0.5 m,
PCL's default size rule.  Every figure is the median of --calls calls after --warmup, with the fastest and slowest call
beside it.  Prints one JSON line.

--cell-div D[,D...]  again under option cluster_cell_div = D (the grid cell is max(automatic, tolerance / D)).
--yardstick N        N rounds per cloud and tolerance of: wm_cluster_extract (k_cluster_link), then the radius outlier
                     filter with counts_out at radius = tolerance (k_outlier_radius<true>: the same walk over the same
                     grid rule without the unions).  Meant to run under `rocprofv3 --kernel-trace --stats`, whose
                     per-kernel times are the comparison -- link / radius is what the unions cost; nothing else is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, cloud, calls, warmup, tolerance):
    for _ in range(warmup):
        ctx.cluster_extract(cloud, tolerance=tolerance)
    dev, host = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = ctx.cluster_extract(cloud, tolerance=tolerance)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(r["kernel_ms"])
    return {"device_ms": round(float(np.median(dev)), 4), "device_ms_min_max": [round(float(min(dev)), 4), round(float(max(dev)), 4)],
            "host_ms": round(float(np.median(host)), 4), "n_finite": int(r["n_finite"]), "components": int(r["n_components"]),
            "clusters": int(r["n_clusters"]), "largest": int(r["largest"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clouds", default="scene_1m,rings_2m_obstacles")
    ap.add_argument("--tolerances", default="0.2,0.5", help="metres, comma separated (one per kernel trace keeps its rows apart)")
    ap.add_argument("--cell-div", default="", help="D[,D...]: again under option cluster_cell_div = D")
    ap.add_argument("--yardstick", type=int, default=0, help="rounds of cluster_extract + radius outlier filter, for a kernel trace")
    a = ap.parse_args()
    TOLERANCES = [float(x) for x in a.tolerances.split(",") if x]
    import torch
    from libwave_amd import capi, synth
    ctx = capi.Context(0)

    def obstacles():
        scan = torch.from_numpy(synth.scene_rings(2_000_000, seed=42)).to("cuda")
        _, kept, _ = ctx.ground_segment_batch([scan], points=True)
        return kept.clone()

    make = {"scene_1m": lambda: torch.from_numpy(synth.scene(1_000_000, seed=42)).to("cuda"), "rings_2m_obstacles": obstacles}
    out = {"metric": "wm_cluster_extract ms per call, cloud in device memory (median of calls)", "calls": a.calls}
    for name in [c for c in a.clouds.split(",") if c]:
        cloud = make[name]()
        torch.cuda.synchronize()
        row = {"points": int(len(cloud))}
        if a.yardstick:
            for tol in TOLERANCES:
                for _ in range(a.yardstick):
                    ctx.cluster_extract(cloud, tolerance=tol)
                    ctx.outlier_filter(cloud, method=1, radius=tol, min_neighbors=5, counts=True)
            row["yardstick_rounds"] = a.yardstick
        else:
            for tol in TOLERANCES:
                row["tolerance_%g" % tol] = timed(ctx, cloud, a.calls, a.warmup, tol)
            for div in [float(x) for x in a.cell_div.split(",") if x]:
                ctx.set_option("cluster_cell_div", div)
                for tol in TOLERANCES:
                    row["tolerance_%g_div%g" % (tol, div)] = timed(ctx, cloud, a.calls, a.warmup, tol)
                ctx.set_option("cluster_cell_div", 2.0)
        out[name] = row
        del cloud
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
