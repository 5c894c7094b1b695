"""wm_cluster_boxes timing: device milliseconds per call (kernel_ms: HIP events from the first launch to the last box),
everything resident in device memory -- the cloud, the member list, the boxes -- on
  scene_0.1   synth.scene(270 000, seed 5) clustered at 0.1 m: 162 250 clusters, most of one or two points
  scene_0.3   the same at 0.3 m: 1 495 clusters, one of them of 264 439 points
  rings_batch the obstacle clusters of --scans ring scans (rings_sensor_frame(130 000, seed 42 + k)) taken straight from
              wm_ground_segment_batch -> wm_cluster_extract_batch's device outputs: points_out and the batch-wide
              offsets, indices == NULL, one call for the clusters of all scans.
Every figure is the median of --calls calls after --warmup, with the fastest and slowest call beside it.  Next to it
the bytes the streaming passes must read divided by that time: "gbps_two_passes" counts 2 x record size x members (a
sums pass and a projection pass: the least any decomposition reads), "passes" says how many this library runs (three:
the AABB has to be complete before the sums are taken from its corner), and "copy_gbps" is wm_debug_copy_bandwidth from
the same run (read + write of a float4 copy kernel).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, cloud, off, idx, calls, warmup):
    t = {}
    for _ in range(warmup):
        ctx.cluster_boxes(cloud, off, idx)
    ms = []
    for _ in range(calls):
        ctx.cluster_boxes(cloud, off, idx, timing=t)
        ms.append(t["kernel_ms"])
    med = float(np.median(ms))
    members = int(len(idx) if idx is not None else len(cloud))
    record = int(cloud.shape[1]) * 4
    return {"device_ms": round(med, 4), "device_ms_min_max": [round(float(min(ms)), 4), round(float(max(ms)), 4)],
            "clusters": int(len(off) - 1), "members": members, "record_bytes": record, "passes": 3,
            "gbps_two_passes": round(2.0 * record * members / (med * 1e-3) / 1e9, 2) if med > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scans", type=int, default=8)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from libwave_amd import capi, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ground_scenes as S
    ctx = capi.Context(0)
    out = {"bench": "wm_cluster_boxes", "calls": a.calls, "warmup": a.warmup}
    scene = torch.from_numpy(synth.scene(270000, seed=5)).cuda()
    for tol in (0.1, 0.3):
        r = ctx.cluster_extract(scene, tolerance=tol, labels=False)  # device outputs: indices and offsets stay there
        row = timed(ctx, scene, r["offsets"], r["indices"], a.calls, a.warmup)
        row["largest"] = int(r["largest"])
        out["scene_%g" % tol] = row
    scans = [torch.from_numpy(S.rings_sensor_frame(130_000, seed=42 + k)).cuda() for k in range(a.scans)]
    _, kept, goff = ctx.ground_segment_batch(scans, points=True)
    slices = [kept[goff[k]:goff[k + 1]] for k in range(a.scans)]
    got, pts, poff = ctx.cluster_extract_batch(slices, points=True, labels=False, tolerance=0.5, min_cluster_size=20)
    d_off = torch.cat([got[k]["offsets"][(1 if k else 0):] + int(poff[k]) for k in range(a.scans)])
    row = timed(ctx, pts, d_off, None, a.calls, a.warmup)
    row["scans"] = a.scans
    out["rings_batch"] = row
    out["copy_gbps"] = round(ctx.copy_bandwidth(), 1)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
