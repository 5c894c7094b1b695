"""wm_ground_segment timing: milliseconds per call (median of at least 200 calls after warm-up) with the cloud in
device memory and on the host, on three workloads -- the reference's fixture after its test's car-box removal
(with the test's YAML), synth.scene_rings(130_000) in the sensor frame (z - 1.73) and the same scene at 1M points
(defaults) -- and the float64 numpy checker's time per call (tests/ground_reference.py: a correctness oracle, NOT
a CPU baseline of the reference's C++, which needs PCL and Eigen).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--checker-reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import ground_reference as G
    import ground_scenes as S
    from libwave_amd import capi
    from libwave_amd.pcd import load_pcd_xyz
    work = {
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
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
