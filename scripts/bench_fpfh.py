"""wm_fpfh_estimate and wm_feature_match timing, device milliseconds (HIP events inside the calls).

Descriptors: wm_fpfh_stats' three stages -- normals_ms (k_normals, the yardstick: the same search on the same grid at
the same k, existing code), spfh_ms (the first pass: search, pair features, counts, lists) and weight_ms (the second
pass) -- with normal_k = feature_k = k, k = 10 and 32, on the target: synth.scene(1M) voxel-filtered at 0.1 m and
0.2 m, and the obstacle points wm_ground_segment keeps from the 64-ring synth.scene_rings(2M).  The clouds are set
anew before every call, so that the normals are estimated every time.  "spfh_over_normals" is the ratio to judge the
first pass by.

Matching: wm_feature_match's kernel_ms (flags, match kernel, finish) at 4k, 20k and 100k descriptor-like rows per side
in device memory, plain and reciprocal, beside the VALU bound na * nb * 99 lane-operations at the FP32 vector rate
(256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz = 78.6e12 lane-operations per second).

Every figure is the median of --calls calls after --warmup, with the fastest and slowest beside it.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def med(v):
    return {"ms": round(float(np.median(v)), 4), "min_max": [round(float(min(v)), 4), round(float(max(v)), 4)]}


def bench_fpfh(ctx, cloud, k, calls, warmup):
    st = {"normals_ms": [], "spfh_ms": [], "weight_ms": []}
    import torch
    out = torch.empty((len(cloud), 33), dtype=torch.float32, device="cuda")
    for it in range(warmup + calls):
        ctx.set_source(cloud)
        ctx.set_target(cloud)
        r = ctx.fpfh(1, normal_k=k, feature_k=k, out=out)
        assert r["rc"] == 0
        if it >= warmup:
            for key in st:
                st[key].append(r[key])
    row = {key: med(v) for key, v in st.items()}
    row["n_valid"] = int(r["n_valid"])
    row["spfh_over_normals"] = round(row["spfh_ms"]["ms"] / row["normals_ms"]["ms"], 3)
    return row


def bench_match(ctx, n, calls, warmup):
    import torch
    rng = np.random.default_rng(n)

    def rows(seed_shift):
        r = np.float32(rng.random((n, 33)) * 100) * (rng.random((n, 33)) < 0.4)
        r[:, 0] += 1 + seed_shift
        return torch.from_numpy(np.ascontiguousarray(r, np.float32)).to("cuda")

    a, b = rows(0), rows(1)
    bound_ms = float(n) * n * 99 / VALU_LANE_OPS_PER_S * 1e3
    out = {"rows_per_side": n, "valu_bound_ms": round(bound_ms, 4)}
    for name, recip in (("plain", False), ("reciprocal", True)):
        ms = []
        for it in range(warmup + calls):
            r = ctx.feature_match(a, b, reciprocal=recip)
            if it >= warmup:
                ms.append(r["kernel_ms"])
        out[name] = med(ms)
        out[name]["over_bound"] = round(out[name]["ms"] / (bound_ms * (2 if recip else 1)), 3)
        out[name]["n_matched"] = int(r["n_matched"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", default="scene_1m_voxel_0.1,scene_1m_voxel_0.2,rings_2m_obstacles")
    ap.add_argument("--k", default="10,32")
    ap.add_argument("--match", default="4000,20000,100000", help="rows per side; empty: skip the matching")
    a = ap.parse_args()
    import torch
    from libwave_amd import capi, synth
    ctx = capi.Context(0)

    def voxel(leaf):
        scene = synth.scene(1_000_000, seed=42)
        scene[:, 2] -= 1.73  # the sensor frame: the scene's ground passes through the origin otherwise
        return ctx.voxel_downsample(scene, leaf)

    def obstacles():
        scan = synth.scene_rings(2_000_000, seed=42)
        _, kept, _ = ctx.ground_segment(scan)
        return np.ascontiguousarray(scan[kept, :3])

    make = {"scene_1m_voxel_0.1": lambda: voxel(0.1), "scene_1m_voxel_0.2": lambda: voxel(0.2), "rings_2m_obstacles": obstacles}
    out = {"metric": "device ms per call (median of calls)", "calls": a.calls}
    for name in [c for c in a.clouds.split(",") if c]:
        cloud = torch.from_numpy(np.ascontiguousarray(make[name](), np.float32)).to("cuda")
        torch.cuda.synchronize()
        row = {"points": int(len(cloud))}
        for k in [int(x) for x in a.k.split(",") if x]:
            row["k%d" % k] = bench_fpfh(ctx, cloud, k, a.calls, a.warmup)
        out[name] = row
        del cloud
    sizes = [int(x) for x in a.match.split(",") if x]
    if sizes:
        out["feature_match"] = [bench_match(ctx, n, a.calls, a.warmup) for n in sizes]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
