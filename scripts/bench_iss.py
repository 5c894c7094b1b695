"""wm_iss_keypoints timing: device milliseconds per call (wm_iss_stats.kernel_ms: HIP events from the cloud's packing to
the keypoint list, the grid build and its two small fetches included) and host milliseconds per call (clock around a
call, which ends in its own synchronise), with the cloud resident in device memory, on synth.scene(1M), on its 0.1 m
voxel-filtered points and on the obstacle points wm_ground_segment keeps from the 64-ring synth.scene_rings(2M).  The
salient radius is 6 x and 10 x the cloud's median nearest-neighbour spacing (a float64 kd-tree over the cloud, asked
about 20 000 of its points), the non-max radius 2/3 of that; gamma 0.975, min_neighbors 5.  Every figure is the median
of --calls calls after --warmup, with the fastest and slowest call beside it; the keypoint counts are printed too.
Prints one JSON line.

--cell-div D[,D...]  the same under option iss_cell_div = D (the grid cell is max(automatic, max radius / D)).
--yardstick N        N rounds of: wm_iss_keypoints, then wm_outlier_filter's radius filter with counts_out at the
                     salient radius and at the non-max radius on the same cloud (k_outlier_radius<true>: the same walk
                     without the sums).  Meant to run under ONE `rocprofv3 --kernel-trace --stats` (no counters beside
                     the trace), whose per-kernel times are the comparison: k_iss_scatter and k_iss_nms beside
                     k_outlier_radius<true>.  Nothing else is timed.
--pipeline           the four-stage recipe (descriptors of all points, keypoints of both clouds, the keypoints' rows
                     matched, the pose from the matches) against the three-stage one (every row matched) on a pair of
                     20 000 points, synth.scene(20000) and itself moved by 40 degrees of yaw and (0.8, 0.6, 0): host ms
                     per stage (clock around calls that end in their own synchronise) and the pose errors."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_spacing(host, sample=20000):
    from scipy.spatial import cKDTree
    c = np.asarray(host[:, :3], np.float64)
    c = c[np.isfinite(c).all(1)]
    q = c[np.random.default_rng(1).choice(len(c), min(sample, len(c)), replace=False)]
    return float(np.median(cKDTree(c).query(q, 2)[0][:, 1]))


def timed(ctx, cloud, calls, warmup, **params):
    for _ in range(warmup):
        ctx.iss_keypoints(cloud, labels=False, **params)
    dev, host = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = ctx.iss_keypoints(cloud, labels=False, **params)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(r["kernel_ms"])
    return {"device_ms": round(float(np.median(dev)), 4), "device_ms_min_max": [round(float(min(dev)), 4), round(float(max(dev)), 4)],
            "host_ms": round(float(np.median(host)), 4), "keypoints": int(r["n_keypoints"]), "salient": int(r["n_salient"]),
            "n_finite": int(r["n_finite"])}


def clock(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms": round(float(np.median(ms)), 4), "min_max": [round(float(min(ms)), 4), round(float(max(ms)), 4)]}


def pipeline(ctx, calls, warmup):
    import torch
    from libwave_amd import synth
    src = np.ascontiguousarray(np.asarray(synth.scene(20000, seed=42))[:, :3], np.float32)
    src[:, 2] -= 1.73  # the sensor frame
    a = math.radians(40.0)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (0.8, 0.6, 0.0)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    s = median_spacing(src)
    radii = dict(salient_radius=6 * s, non_max_radius=4 * s)
    dsrc, dtgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    fs = torch.empty((len(src), 33), dtype=torch.float32, device="cuda")
    ft = torch.empty((len(tgt), 33), dtype=torch.float32, device="cuda")
    ctx.set_source(dsrc)
    ctx.set_target(dtgt)

    def describe():
        ctx.set_source(dsrc)
        ctx.set_target(dtgt)
        assert ctx.fpfh(0, out=fs)["rc"] == 0 and ctx.fpfh(1, out=ft)["rc"] == 0

    def err(Tg):
        if Tg is None:
            return None
        dR = Tg[:3, :3].T @ T[:3, :3]
        return [float(np.linalg.norm(Tg[:3, 3] - T[:3, 3])), float(math.acos(max(-1.0, min(1.0, (np.trace(dR) - 1) / 2))))]

    out = {"points": len(src), "median_spacing": round(s, 4)}
    _, out["descriptors"] = clock(describe, calls, warmup)
    # three stages: every row matched
    m3, out["match_all_rows"] = clock(lambda: ctx.feature_match(fs, ft, reciprocal=True), calls, warmup)
    r3, out["pose_all_rows"] = clock(lambda: ctx.corr_ransac(dsrc, dtgt, m3["idx"], refine_model=1, labels=False), calls, warmup)
    out["three_stage"] = {"matches": int(m3["n_matched"]), "kept": int(r3["n_out"]), "pose_error_m_rad": err(r3["T"])}

    # four stages: keypoints in between
    def detect():
        return ctx.iss_keypoints(dsrc, labels=False, **radii), ctx.iss_keypoints(dtgt, labels=False, **radii)

    (ks, kt), out["keypoints"] = clock(detect, calls, warmup)

    def match():
        a_, b_ = ctx.gather_records(fs, ks["indices"]), ctx.gather_records(ft, kt["indices"])
        return ctx.feature_match(a_, b_, reciprocal=True)

    m4, out["gather_and_match_keypoint_rows"] = clock(match, calls, warmup)
    found = m4["idx"] >= 0
    query = ks["indices"][found].contiguous()
    match_idx = kt["indices"][m4["idx"][found].long()].contiguous()
    torch.cuda.synchronize()
    r4, out["pose_keypoint_rows"] = clock(lambda: ctx.corr_ransac(dsrc, dtgt, match_idx, query, refine_model=1, labels=False),
                                          calls, warmup)
    out["four_stage"] = {"keypoints": [int(ks["n_out"]), int(kt["n_out"])], "matches": int(m4["n_matched"]), "kept": int(r4["n_out"]),
                         "pose_error_m_rad": err(r4["T"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", default="scene_1m,scene_1m_voxel_0.1,rings_2m_obstacles")
    ap.add_argument("--radii", default="6,10", help="salient radius in median spacings")
    ap.add_argument("--cell-div", default="", help="D[,D...]: the same under option iss_cell_div = D")
    ap.add_argument("--yardstick", type=int, default=0, help="rounds of iss_keypoints + the radius filter, for a kernel trace")
    ap.add_argument("--pipeline", action="store_true", help="the four-stage recipe against the three-stage one")
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

    make = {"scene_1m": lambda: synth.scene(1_000_000, seed=42), "scene_1m_voxel_0.1": lambda: voxel(0.1),
            "rings_2m_obstacles": obstacles}
    out = {"metric": "wm_iss_keypoints ms per call, cloud in device memory (median of calls)", "calls": a.calls}
    mult = [float(x) for x in a.radii.split(",") if x]
    for name in [c for c in a.clouds.split(",") if c]:
        host = np.ascontiguousarray(np.asarray(make[name]())[:, :3], np.float32)
        s = median_spacing(host)
        cloud = torch.from_numpy(host).to("cuda")
        torch.cuda.synchronize()
        row = {"points": int(len(host)), "median_spacing": round(s, 5)}
        for k in mult:
            radii = dict(salient_radius=k * s, non_max_radius=k * s * 2.0 / 3.0)
            if a.yardstick:
                for _ in range(a.yardstick):
                    ctx.iss_keypoints(cloud, labels=False, **radii)
                    for r in radii.values():
                        ctx.outlier_filter(cloud, method=1, radius=r, min_neighbors=5, counts=True)
                row["yardstick_rounds"] = a.yardstick
                continue
            row["salient_%gx" % k] = timed(ctx, cloud, a.calls, a.warmup, **radii)
            for div in [float(x) for x in a.cell_div.split(",") if x]:
                ctx.set_option("iss_cell_div", div)
                row["salient_%gx_div%g" % (k, div)] = timed(ctx, cloud, a.calls, a.warmup, **radii)
                ctx.set_option("iss_cell_div", 2.0)
        out[name] = row
        del cloud
    if a.pipeline:
        out["pipeline"] = pipeline(ctx, a.calls, a.warmup)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
