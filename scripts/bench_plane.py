#!/usr/bin/env python3
"""Point-to-plane against point-to-point ICP on one MI355X, same commit: iterations and milliseconds to converge,
free-running with the stopping criteria of tests/golden/config/icp.yaml, on the 1M <-> 1M bench pair
(synth.pair_tiled(points, 1, seed=42): bench.py's) and the 64-ring pair (synth.pair(points, seed=42,
pattern="rings")).  A registration is wm_set_source + wm_set_target + wm_icp_align with both clouds resident in device
memory -- so the plane figure INCLUDES the target's normals (estimated once per target) -- timed by the host clock around
calls that end in their own synchronise.  The two metrics alternate (svd, plane, svd, plane ...) after a warm-up of
both; per metric: iterations, median [min ... max] ms of --runs registrations, and the device time of the plane
metric's normals alone (wm_estimate_normals on a fresh target).  Prints one JSON line.

The claim under test: fewer iterations x a dearer iteration (a search-only launch, the plane sums, a solve) < before."""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YAML = dict(max_corr=3.0, max_iter=100, t_eps=1e-8, fit_eps=1e-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop", type=int, default=0, help="profiling aid: this many extra plane registrations of the first pair, nothing timed")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from libwave_amd import capi, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane.py needs a GPU: there is no fallback")
    pairs = {"bench_pair": synth.pair_tiled(a.points, 1, seed=42), "rings64": synth.pair(a.points, seed=42, pattern="rings")}
    out = {"points": a.points, "runs": a.runs, "criteria": YAML, "timing": "host clock around set_source + set_target + icp_align, "
           "device-resident clouds; plane includes the normals"}
    ctx = capi.Context(0)
    for name, (ref, tgt, T_gt) in pairs.items():
        d_ref = torch.from_numpy(ref).to("cuda")
        d_tgt = torch.from_numpy(tgt).to("cuda")
        torch.cuda.synchronize()

        def reg(mode):
            t0 = time.perf_counter()
            ctx.set_source(d_ref)
            ctx.set_target(d_tgt)
            r = ctx.icp_align(mode=mode, nn_method=capi.WM_NN_GRID, carry_state=0, **YAML)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        modes = (("svd", capi.WM_ICP_SVD), ("plane", capi.WM_ICP_PLANE))
        for _ in range(a.warmup):
            for _, m in modes:
                reg(m)
        if a.loop:
            for _ in range(a.loop):
                reg(capi.WM_ICP_PLANE)
            continue
        ms = {k: [] for k, _ in modes}
        last = {}
        for _ in range(a.runs):
            for k, m in modes:
                t, r = reg(m)
                assert r["rc"] == 0, r
                ms[k].append(t)
                last[k] = r
        normals_ms = []
        buf = torch.empty((len(tgt), 4), dtype=torch.float32, device="cuda")
        for _ in range(a.runs):
            ctx.set_source(d_ref)
            ctx.set_target(d_tgt)
            ctx.sizes()  # (the clouds' pending set-up is not the normals')
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.estimate_normals(1, 0, out=buf)
            normals_ms.append((time.perf_counter() - t0) * 1e3)
        res = {}
        for k, _ in modes:
            v = sorted(ms[k])
            r = last[k]
            res[k] = {"iterations": r["iterations"], "state": r["state"], "ms_median": round(float(np.median(v)), 3),
                      "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "ms_each": [round(x, 3) for x in ms[k]],
                      "err_vs_truth_F": float(np.linalg.norm(r["T"] - T_gt))}
        res["plane"]["normals_ms_median"] = round(float(np.median(normals_ms)), 3)
        res["plane_over_svd"] = round(res["plane"]["ms_median"] / res["svd"]["ms_median"], 3)
        out[name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
