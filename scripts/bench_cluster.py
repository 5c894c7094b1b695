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
                     per-kernel times are the comparison -- link / radius is what the unions cost; nothing else is timed.
--batch S[,S...]     adds the key "batch": wm_cluster_extract_batch over S scans against the same S scans through
                     wm_cluster_extract one after the other on the same context, the two alternating; ms PER SCAN, the
                     median of --rounds rounds, one entry per repeat (--repeats).  Device input, tolerance 0.2 and
                     0.5 m; the scans: the obstacle points wm_ground_segment_batch keeps from
                     rings_sensor_frame(130 000, seed 42 + k), and the 3 000-point stress shapes of the tests in turn.
                     --skip-plain leaves the single-call part out.
--cond               per cloud and tolerance, in place of the plain rows: wm_cluster_extract_cond with the normal test
                     (normals from wm_estimate_normals with k = 10 on a second context, left in device memory; angle
                     30 degrees) beside wm_cluster_extract on the same cloud, the two alternating call by call -- device
                     ms per call of each and their ratio -- and wm_estimate_normals alone beside them: host ms around
                     the call on a freshly set target (the target's grid is built inside it), which ends in its own
                     synchronise.  Under `rocprofv3 --kernel-trace --stats` the two k_cluster_link instantiations have
                     rows of their own."""
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


def timed_cond(ctx, nctx, cloud, calls, warmup, tolerance, k=10, angle_deg=30.0):
    import torch
    attr = torch.empty((len(cloud), 4), dtype=torch.float32, device=cloud.device)
    normals = []
    for i in range(min(calls, 10) + 1):
        nctx.set_source(cloud[:1000])  # (wm_estimate_normals wants both clouds; only the target's normals are made)
        nctx.set_target(cloud)
        nctx.sizes()  # (the clouds' pending set-up is not the normals')
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nctx.estimate_normals(1, k, out=attr)
        if i:
            normals.append((time.perf_counter() - t0) * 1e3)
    angle = float(np.deg2rad(angle_deg))
    for _ in range(warmup):
        ctx.cluster_extract(cloud, tolerance=tolerance)
        ctx.cluster_extract_cond(cloud, attr, tolerance=tolerance, max_normal_angle=angle)
    plain, cond = [], []
    for _ in range(calls):
        r = ctx.cluster_extract(cloud, tolerance=tolerance)
        plain.append(r["kernel_ms"])
        rc = ctx.cluster_extract_cond(cloud, attr, tolerance=tolerance, max_normal_angle=angle)
        cond.append(rc["kernel_ms"])

    def cell(ms, res):
        return {"device_ms": round(float(np.median(ms)), 4), "device_ms_min_max": [round(float(min(ms)), 4), round(float(max(ms)), 4)],
                "components": int(res["n_components"]), "largest": int(res["largest"])}
    return {"n_finite": int(r["n_finite"]), "normal_k": k, "max_normal_angle_deg": angle_deg, "plain": cell(plain, r),
            "cond": cell(cond, rc), "cond_over_plain": round(float(np.median(cond) / np.median(plain)), 4),
            "estimate_normals_host_ms": round(float(np.median(normals)), 4),
            "estimate_normals_host_ms_min_max": [round(float(min(normals)), 4), round(float(max(normals)), 4)]}


def bench_batch(ctx, sizes, rounds, warmup, repeats, tolerances):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ground_scenes as S
    import knn_reference as KR
    top = max(sizes)
    rings = []
    for k0 in range(0, top, 8):  # (eight scans per filter call: the ground workspace stays small)
        scans = [torch.from_numpy(S.rings_sensor_frame(130_000, 42 + k)).to("cuda") for k in range(k0, min(k0 + 8, top))]
        _, kept, offs = ctx.ground_segment_batch(scans, points=True)
        rings += [kept[offs[j]:offs[j + 1]].clone() for j in range(len(scans))]
    shapes = KR.shapes()
    stress = [torch.from_numpy(np.ascontiguousarray(shapes[KR.NAMES[k % len(KR.NAMES)]])).to("cuda") for k in range(top)]
    work = {"rings_130k_obstacles": rings, "stress_3000": stress}
    out = {"metric": "ms per scan (median of rounds; one entry per repeat)", "rounds": rounds, "repeats": repeats}
    for name, scans in work.items():
        out[name] = {"points_per_scan": int(np.mean([len(s) for s in scans]))}
    torch.cuda.synchronize()
    for _ in range(repeats):  # the whole measurement, again
        for name, scans in work.items():
            for tol in tolerances:
                for S_ in sizes:
                    clouds = scans[:S_]
                    for _ in range(max(warmup // S_, 3)):
                        for c in clouds:
                            ctx.cluster_extract(c, tolerance=tol)
                        ctx.cluster_extract_batch(clouds, tolerance=tol)
                    tl, tb = [], []
                    for _ in range(rounds):
                        t0 = time.perf_counter()
                        for c in clouds:
                            ctx.cluster_extract(c, tolerance=tol)
                        t1 = time.perf_counter()
                        ctx.cluster_extract_batch(clouds, tolerance=tol)
                        t2 = time.perf_counter()
                        tl.append((t1 - t0) * 1e3 / S_)
                        tb.append((t2 - t1) * 1e3 / S_)
                    cell = out[name].setdefault("tolerance_%g_S%d" % (tol, S_), {"loop_ms_per_scan": [], "batch_ms_per_scan": []})
                    cell["loop_ms_per_scan"].append(round(float(np.median(tl)), 4))
                    cell["batch_ms_per_scan"].append(round(float(np.median(tb)), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="", help="S[,S...]: also time wm_cluster_extract_batch against a loop of single calls")
    ap.add_argument("--rounds", type=int, default=200, help="rounds of a --batch cell")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of the whole --batch measurement")
    ap.add_argument("--skip-plain", action="store_true", help="with --batch: leave the single-call part out")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clouds", default="scene_1m,rings_2m_obstacles")
    ap.add_argument("--tolerances", default="0.2,0.5", help="metres, comma separated (one per kernel trace keeps its rows apart)")
    ap.add_argument("--cell-div", default="", help="D[,D...]: again under option cluster_cell_div = D")
    ap.add_argument("--cond", action="store_true", help="wm_cluster_extract_cond (normals, k = 10, 30 degrees) beside wm_cluster_extract")
    ap.add_argument("--yardstick", type=int, default=0, help="rounds of cluster_extract + radius outlier filter, for a kernel trace")
    a = ap.parse_args()
    TOLERANCES = [float(x) for x in a.tolerances.split(",") if x]
    import torch
    from libwave_amd import capi, synth
    ctx = capi.Context(0)
    nctx = capi.Context(0) if a.cond else None  # the normals' context: a registration state of its own

    def obstacles():
        scan = torch.from_numpy(synth.scene_rings(2_000_000, seed=42)).to("cuda")
        _, kept, _ = ctx.ground_segment_batch([scan], points=True)
        return kept.clone()

    make = {"scene_1m": lambda: torch.from_numpy(synth.scene(1_000_000, seed=42)).to("cuda"), "rings_2m_obstacles": obstacles}
    out = {"metric": "wm_cluster_extract ms per call, cloud in device memory (median of calls)", "calls": a.calls}
    sizes = [int(x) for x in a.batch.split(",") if x]
    for name in [c for c in a.clouds.split(",") if c and not (sizes and a.skip_plain)]:
        cloud = make[name]()
        torch.cuda.synchronize()
        row = {"points": int(len(cloud))}
        if a.yardstick:
            for tol in TOLERANCES:
                for _ in range(a.yardstick):
                    ctx.cluster_extract(cloud, tolerance=tol)
                    ctx.outlier_filter(cloud, method=1, radius=tol, min_neighbors=5, counts=True)
            row["yardstick_rounds"] = a.yardstick
        elif a.cond:
            for tol in TOLERANCES:
                row["tolerance_%g" % tol] = timed_cond(ctx, nctx, cloud, a.calls, a.warmup, tol)
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
    if sizes:
        out["batch"] = bench_batch(ctx, sizes, a.rounds, a.warmup, a.repeats, TOLERANCES)
    ctx.close()
    if nctx:
        nctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
