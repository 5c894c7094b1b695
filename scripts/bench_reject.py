#!/usr/bin/env python3
"""Correspondence rejection in ICP on one MI355X, same commit: what it buys and what an iteration of it costs.

Pairs: the partial-overlap pair (synth.pair(points, mode="resample") under the pose (0.5, -0.3, 0.05) m / (0.01, -0.02,
0.04) rad, the source cut to x < 15 m in the reference frame, the target to the points whose pre-image has x > -15 m:
about 46 % overlap) and the full-overlap bench pair (synth.pair_tiled(points, 1, seed=42): bench.py's).

  converge   free-running, max_corr 3, max_iter 100, t_eps 1e-8, fit_eps 1e-6: iterations, stop state and the distance
             of the final pose from the true one, without rejection, trimmed 0.5 and median 1.0
  per_iter   force_iterations = 30, both clouds resident: device ms per iteration (wm_icp_stats.align_ms / 30, median of
             --runs) for rejection off, trimmed 0.5, median 1.0 and WM_ICP_PLANE without rejection -- the plane metric
             has the same launch shape (a search-only launch, a streaming sums pass, a solve), so it is the yardstick on
             the same commit; with profile = 2 the split of an iteration into search (nn_ms + coarse_ms), select + sums
             (stats_ms: the three histogram passes and the filtered sums of a rejecting iteration) and solve

Prints one JSON line."""
import argparse
import json
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "4")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CRITERIA = dict(max_corr=3.0, max_iter=100, t_eps=1e-8, fit_eps=1e-6)
PARTIAL_T = ((0.5, -0.3, 0.05), (0.01, -0.02, 0.04))
FORCED = 30


def partial_pair(synth, n, cut=15.0):
    T = synth.make_T(*PARTIAL_T)
    ref, tgt, T_gt = synth.pair(n, mode="resample", T=T)
    pre = synth.transform_points(tgt, np.linalg.inv(T_gt))
    return ref[ref[:, 0] < cut].copy(), tgt[pre[:, 0] > -cut].copy(), T_gt


def pose_error(Ta, Tb):
    dt = float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))
    R = Ta[:3, :3].T @ Tb[:3, :3]
    return dt, float(2.0 * np.arcsin(min(1.0, np.linalg.norm(R - np.eye(3)) / (2.0 * np.sqrt(2.0)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    from libwave_amd import capi, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_reject.py needs a GPU: there is no fallback")
    pairs = {"partial_overlap": partial_pair(synth, a.points), "bench_pair": synth.pair_tiled(a.points, 1, seed=42)}
    variants = (("off", dict()), ("trimmed_0.5", dict(reject=capi.WM_REJECT_TRIMMED, reject_ratio=0.5)),
                ("median_1.0", dict(reject=capi.WM_REJECT_MEDIAN, reject_factor=1.0)), ("plane_off", dict(mode=capi.WM_ICP_PLANE)))
    out = {"points": a.points, "runs": a.runs, "criteria": CRITERIA, "forced_iterations": FORCED}
    ctx = capi.Context(0)
    for name, (ref, tgt, T_gt) in pairs.items():
        d_ref = torch.from_numpy(ref).to("cuda")
        d_tgt = torch.from_numpy(tgt).to("cuda")
        torch.cuda.synchronize()
        ctx.set_source(d_ref)
        ctx.set_target(d_tgt)
        res = {"n_source": len(ref), "n_target": len(tgt), "converge": {}, "per_iter": {}}
        for vname, kw in variants[:3]:
            r = ctx.icp_align(nn_method=capi.WM_NN_GRID, carry_state=0, **kw, **CRITERIA)
            row = {"rc": r["rc"], "iterations": r["iterations"], "state": r["state"], "n_corr": r["n_corr"], "n_matched": r["n_matched"],
                   "align_ms": round(r["align_ms"], 3)}
            if r["T"] is not None:
                dt, ang = pose_error(r["T"], T_gt)
                row.update(err_m=dt, err_rad=ang)
            res["converge"][vname] = row
        for vname, kw in variants:
            forced = dict(CRITERIA, force_iterations=FORCED, nn_method=capi.WM_NN_GRID, carry_state=0, **kw)
            for _ in range(a.warmup):
                ctx.icp_align(**forced)
            ms = []
            for _ in range(a.runs):
                r = ctx.icp_align(**forced)
                assert r["rc"] == 0 and r["iterations"] == FORCED, r
                ms.append(r["align_ms"] / FORCED)
            r = ctx.icp_align(profile=2, **forced)
            v = sorted(ms)
            res["per_iter"][vname] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                                      "profile2_ms": {"search": round((r["nn_ms"] + r["coarse_ms"]) / FORCED, 4),
                                                      "select_and_sums": round(r["stats_ms"] / FORCED, 4),
                                                      "solve": round(r["solve_ms"] / FORCED, 4)}}
        out[name] = res
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
