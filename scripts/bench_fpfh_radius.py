"""wm_fpfh_radius timing, device milliseconds (HIP events inside the call): wm_fpfh_radius_stats' stages -- normals_ms
(k_nr_sums and k_nr_finish at the normal radius), spfh_ms (the first walk: pair features, counts) and weight_ms (the
second walk) -- and kernel_ms, the whole call from the cloud's packing on (grid build and its fetches included), with
the cloud resident in device memory, on the clouds scripts/bench_fpfh.py uses: synth.scene(1M) voxel-filtered at 0.1 m
and 0.2 m, and the obstacle points wm_ground_segment keeps from the 64-ring synth.scene_rings(2M).  The feature radius
is 6 x and 10 x the cloud's median nearest-neighbour spacing (a float64 kd-tree over the cloud, asked about 20 000 of
its points), the normal radius half of it.  Every figure is the median of --calls calls after --warmup, with the
fastest and slowest beside it; max_neighbors and n_valid are printed too (a cloud with a point above 8191 neighbours
is refused: "rc" says so).  Prints one JSON line.

--cell-div D[,D...]  the same under option fpfh_cell_div = D (the grid cell is max(automatic, max radius / D)).
--yardstick N        N rounds of: wm_normals_radius at the FEATURE radius, wm_fpfh_radius with those normals given, and
                     wm_iss_keypoints with its salient radius at the feature radius under iss_cell_div = the current
                     fpfh_cell_div -- the same walk on the same grid with six sums (k_iss_scatter).  Meant to run under
                     ONE `rocprofv3 --kernel-trace --stats` (no counters beside the trace), whose per-kernel times are
                     the comparison: k_nr_sums, k_spfh_radius and k_fpfh_weight_radius beside k_iss_scatter.  Nothing
                     else is timed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("normals_ms", "spfh_ms", "weight_ms", "kernel_ms")


def median_spacing(host, sample=20000):
    from scipy.spatial import cKDTree
    c = np.asarray(host[:, :3], np.float64)
    c = c[np.isfinite(c).all(1)]
    q = c[np.random.default_rng(1).choice(len(c), min(sample, len(c)), replace=False)]
    return float(np.median(cKDTree(c).query(q, 2)[0][:, 1]))


def med(v):
    return {"ms": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def timed(ctx, cloud, out, calls, warmup, rf):
    r = None
    for _ in range(warmup):
        r = ctx.fpfh_radius(cloud, rf, normal_radius=0.5 * rf, out=out)
        if r["rc"] != 0:
            return {"rc": int(r["rc"]), "max_neighbors": int(r["max_neighbors"])}
    t = {s: [] for s in STAGES}
    for _ in range(calls):
        r = ctx.fpfh_radius(cloud, rf, normal_radius=0.5 * rf, out=out)
        for s in STAGES:
            t[s].append(r[s])
    row = {s: med(t[s]) for s in STAGES}
    row.update(rc=int(r["rc"]), max_neighbors=int(r["max_neighbors"]), n_valid=int(r["n_valid"]), n_finite=int(r["n_finite"]),
               weight_over_spfh=round(row["weight_ms"]["ms"] / row["spfh_ms"]["ms"], 3))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", default="scene_1m_voxel_0.1,scene_1m_voxel_0.2,rings_2m_obstacles")
    ap.add_argument("--radii", default="6,10", help="feature radius in median spacings; the normal radius is half of it")
    ap.add_argument("--cell-div", default="", help="D[,D...]: the same under option fpfh_cell_div = D")
    ap.add_argument("--yardstick", type=int, default=0, help="rounds of the walks beside k_iss_scatter, for a kernel trace")
    a = ap.parse_args()
    import torch
    from libwave_amd import capi, synth
    ctx = capi.Context(0)

    def voxel(leaf):
        scene = synth.scene(1_000_000, seed=42)
        return ctx.voxel_downsample(scene, leaf)

    def obstacles():
        scan = synth.scene_rings(2_000_000, seed=42)
        _, kept, _ = ctx.ground_segment(scan)
        return np.ascontiguousarray(scan[kept, :3])

    make = {"scene_1m_voxel_0.1": lambda: voxel(0.1), "scene_1m_voxel_0.2": lambda: voxel(0.2), "rings_2m_obstacles": obstacles}
    out = {"metric": "wm_fpfh_radius device ms per call, cloud in device memory (median of calls)", "calls": a.calls}
    mult = [float(x) for x in a.radii.split(",") if x]
    divs = [float(x) for x in a.cell_div.split(",") if x]
    for name in [c for c in a.clouds.split(",") if c]:
        host = np.ascontiguousarray(np.asarray(make[name]())[:, :3], np.float32)
        s = median_spacing(host)
        cloud = torch.from_numpy(host).to("cuda")
        rows = torch.empty((len(host), 33), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        row = {"points": int(len(host)), "median_spacing": round(s, 5)}
        for k in mult:
            rf = k * s
            if a.yardstick:
                div = divs[0] if divs else 2.0
                ctx.set_option("fpfh_cell_div", div)
                ctx.set_option("iss_cell_div", div)
                for _ in range(a.yardstick):
                    nrm = ctx.normals_radius(cloud, rf)["normals"]
                    ctx.fpfh_radius(cloud, rf, normals=nrm, out=rows)
                    ctx.iss_keypoints(cloud, labels=False, salient_radius=rf, non_max_radius=0.5 * rf)
                ctx.set_option("fpfh_cell_div", 2.0)
                ctx.set_option("iss_cell_div", 2.0)
                row["yardstick_rounds"] = a.yardstick
                continue
            row["feature_%gx" % k] = timed(ctx, cloud, rows, a.calls, a.warmup, rf)
            for div in divs:
                ctx.set_option("fpfh_cell_div", div)
                row["feature_%gx_div%g" % (k, div)] = timed(ctx, cloud, rows, a.calls, a.warmup, rf)
                ctx.set_option("fpfh_cell_div", 2.0)
        out[name] = row
        del cloud, rows
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
