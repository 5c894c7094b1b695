"""wm_ground_segment timing: milliseconds per call (median of at least 200 calls after warm-up) with the cloud in
device memory and on the host, on three workloads -- the reference's fixture after its test's car-box removal
(with the test's YAML), synth.scene_rings(130_000) in the sensor frame (z - 1.73) and the same scene at 1M points
(defaults) -- and the float64 numpy checker's time per call (tests/ground_reference.py: a correctness oracle, NOT
a CPU baseline of the reference's C++, which needs PCL and Eigen).  Prints one JSON line.

--batch S[,S...] adds the key "batch": wm_ground_segment_batch against the same scans through wm_ground_segment one
by one on the same context, milliseconds PER SCAN.  Loop and batch alternate (loop, batch, loop, batch ...) after a
warm-up of both; the figure is the median of --calls rounds, each timed by the host clock around calls that end in
their own synchronise; the whole measurement is repeated --repeats times and every repeat's median is reported, so
the spread of the repeats is the noise a comparison has to beat.  Workloads: a drive of the fixture (the scan moved
by step k: yaw 0.01 k rad, then (0.2 k, 0.05 k, 0) m; 8 steps, cycled to S scans) with the test's YAML, and
rings_sensor_frame(130_000, seed = 42 + k) with the defaults.  --skip-plain leaves the single-call part out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def drive_scans(fixture, steps=8):
    out = []
    for k in range(steps):
        c, s = np.cos(0.01 * k), np.sin(0.01 * k)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        p = fixture.astype(np.float64) @ R.T + np.array([0.2 * k, 0.05 * k, 0.0])
        out.append(np.ascontiguousarray(p.astype(np.float32)))
    return out


def bench_batch(ctx, sizes, calls, warmup, repeats, fixture, yaml_params, default_params, rings):
    import torch
    drive = drive_scans(fixture)
    top = max(sizes)
    work = {
        "fixture_drive": ([drive[k % len(drive)] for k in range(top)], yaml_params),
        "rings_130k": ([rings(130_000, 42 + k) for k in range(top)], default_params),
    }
    out = {"metric": "ms per scan (median of rounds; one entry per repeat)", "rounds": calls, "repeats": repeats}
    dev = {}
    for name, (scans, P) in work.items():
        dev[name] = [torch.from_numpy(s).to("cuda") for s in scans]
        out[name] = {"points_per_scan": int(np.mean([len(s) for s in scans]))}
    torch.cuda.synchronize()
    for _ in range(repeats):  # the whole measurement, again
        for name, (scans, P) in work.items():
            for S in sizes:
                for where, clouds in (("device", dev[name][:S]), ("host", scans[:S])):
                    for _ in range(max(warmup // S, 3)):
                        for c in clouds:
                            ctx.ground_segment(c, P)
                        ctx.ground_segment_batch(clouds, P)
                    tl, tb = [], []
                    for _ in range(calls):
                        t0 = time.perf_counter()
                        for c in clouds:
                            ctx.ground_segment(c, P)
                        t1 = time.perf_counter()
                        ctx.ground_segment_batch(clouds, P)
                        t2 = time.perf_counter()
                        tl.append((t1 - t0) * 1e3 / S)
                        tb.append((t2 - t1) * 1e3 / S)
                    cell = out[name].setdefault("S%d_%s" % (S, where), {"loop_ms_per_scan": [], "batch_ms_per_scan": []})
                    cell["loop_ms_per_scan"].append(round(float(np.median(tl)), 4))
                    cell["batch_ms_per_scan"].append(round(float(np.median(tb)), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="", help="S[,S...]: also time wm_ground_segment_batch against a loop of single calls")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of the whole --batch measurement")
    ap.add_argument("--skip-plain", action="store_true", help="with --batch: leave the single-call part out")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--checker-reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import ground_reference as G
    import ground_scenes as S
    from libwave_amd import capi
    from libwave_amd.pcd import load_pcd_xyz
    sizes = [int(x) for x in a.batch.split(",") if x]
    work = {} if (sizes and a.skip_plain) else {
        "fixture_50k": (G.car_box_removal(load_pcd_xyz(os.path.join(ROOT, "tests", "golden", "testscan.pcd"))),
                        G.load_yaml(S.YAML)),
        "rings_130k": (S.rings_sensor_frame(130_000), G.default_params()),
        "rings_1m": (S.rings_sensor_frame(1_000_000), G.default_params()),
    }
    ctx = capi.Context(0)
    out = {"metric": "wm_ground_segment ms per call (median)", "calls": a.calls}
    for name, (pts, P) in work.items():
        row = {"points": int(len(pts))}
        for where, cloud in (("device", torch.from_numpy(pts).to("cuda")), ("host", pts)):
            for _ in range(a.warmup):
                ctx.ground_segment(cloud, P)
            ts = []
            for _ in range(a.calls):
                t0 = time.perf_counter()
                ctx.ground_segment(cloud, P)
                ts.append((time.perf_counter() - t0) * 1e3)
            row[where + "_ms"] = round(float(np.median(ts)), 4)
        ts = []
        for _ in range(a.checker_reps):
            t0 = time.perf_counter()
            G.segment(pts, P)
            ts.append((time.perf_counter() - t0) * 1e3)
        row["numpy_checker_ms"] = round(float(np.median(ts)), 1)
        row["stats"] = ctx.ground_segment(pts, P)[2]
        out[name] = row
    if sizes:
        fixture = G.car_box_removal(load_pcd_xyz(os.path.join(ROOT, "tests", "golden", "testscan.pcd")))
        out["batch"] = bench_batch(ctx, sizes, a.calls, a.warmup, a.repeats, fixture, G.load_yaml(S.YAML),
                                   G.default_params(), S.rings_sensor_frame)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
