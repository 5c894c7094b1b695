"""wm_corr_ransac timing: device milliseconds per call (wm_corr_ransac_stats.kernel_ms: HIP events from the front to
the last output, the rounds' fetches and the refit's included) and host milliseconds per call (clock around a call, which
ends in its own synchronise), clouds and correspondences resident in device memory, at m = 4 000, 20 000, 100 000 and
1 000 000 correspondences of which 10 % and 50 % are planted inliers of one pose (the rest pair uniform points of a
20 m box), max_iterations 1000, PCL's other defaults, seed 0, refine_model 0 and 1.  Every figure is the median of
--calls calls after --warmup, with the fastest and slowest call beside it; the loop's counters say how much work a call
was.  "pair_tests" is iterations x valid pairs: the tests of the entries the loop consumed.  It is every test the device
made when the loop ran to max_iterations (10 % inliers: a round never holds more entries than the loop can still
count); when the loop stops inside a round (50 % inliers: after some 35 of the round's 256 entries) the device has
tested the rest of that round too and the number is a lower bound.  "tests_per_s" divides it by the device time of the
WHOLE call; "unfused_fraction" is 26 operations a test against 78.6e12 unfused float operations per second (DESIGN.md
4.11).  Prints one JSON line.

--yardstick N   N calls of wm_corr_ransac at m = 1 000 000 with 10 % inliers and min_sample_distance 0 (no entry is
                skipped, so the pair tests are exact), and N of wm_sac_segment on synth.scene(1M) at threshold 0.2 m,
                max_iterations 1000.  Meant to run under `rocprofv3 --kernel-trace --stats` in a run of its own, with no
                counters: its per-kernel times put k_corr_count beside k_sac_count from one trace.  The JSON line
                carries the pair tests and the plane tests the N calls made; nothing is timed here."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_TEST = 26
UNFUSED_OPS_PER_S = 78.6e12


def planted(m, share, thr, seed):
    """src, tgt float32 (m, 3), match int32 (m,): entry e pairs source e with target e"""
    rng = np.random.default_rng(seed)
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ang = math.radians(40.0)
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    src = rng.uniform(-10, 10, (m, 3))
    tgt = rng.uniform(-10, 10, (m, 3))
    good = rng.permutation(m) < int(round(share * m))
    tgt[good] = src[good] @ R.T + [4.0 / 3, -2.0 / 3, 4.0 / 3] + rng.uniform(-thr / 8, thr / 8, (int(good.sum()), 3))
    return src.astype(np.float32), tgt.astype(np.float32), np.arange(m, dtype=np.int32)


def entries_evaluated(rounds, max_it, round_max=256):
    """the rounds' sizes while no entry is skipped: R = min(round_max, max_it + 1 - it)"""
    total = it = 0
    for _ in range(rounds):
        r = min(round_max, max_it + 1 - it)
        total += r
        it += r
    return total


def timed(ctx, args, calls, warmup, **kw):
    for _ in range(warmup):
        ctx.corr_ransac(*args, labels=False, **kw)
    dev, host = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = ctx.corr_ransac(*args, labels=False, **kw)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(r["kernel_ms"])
    ms = float(np.median(dev))
    tests = r["iterations"] * r["n_valid"]
    return {"device_ms": round(ms, 4), "device_ms_min_max": [round(float(min(dev)), 4), round(float(max(dev)), 4)],
            "host_ms": round(float(np.median(host)), 4), "rc": int(r["rc"]), "iterations": int(r["iterations"]),
            "skipped": int(r["skipped"]), "rounds": int(r["rounds"]), "entries": int(r["hypotheses"]),
            "inliers": int(r["n_out"]), "refined": int(r["refined"]), "pair_tests": int(tests),
            "tests_per_s": round(tests / (ms * 1e-3), 1) if ms > 0 else None,
            "unfused_fraction": round(tests * OPS_PER_TEST / (ms * 1e-3) / UNFUSED_OPS_PER_S, 4) if ms > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="4000,20000,100000,1000000")
    ap.add_argument("--shares", default="0.1,0.5")
    ap.add_argument("--yardstick", type=int, default=0, help="calls of corr_ransac and sac_segment, for a kernel trace")
    a = ap.parse_args()
    import torch
    from libwave_amd import capi, synth
    ctx = capi.Context(0)
    thr = 0.05
    if a.yardstick:
        src, tgt, mi = (torch.from_numpy(x).to("cuda") for x in planted(1_000_000, 0.1, thr, 1))
        torch.cuda.synchronize()
        tests = 0
        for _ in range(a.yardstick):
            r = ctx.corr_ransac(src, tgt, mi, labels=False, max_iterations=1000, min_sample_distance=0.0)
            tests += entries_evaluated(r["rounds"], 1000) * r["n_valid"]
        out = {"yardstick_calls": a.yardstick,
               "corr": {"pairs": int(r["n_valid"]), "pair_tests": int(tests), "skipped": int(r["skipped"]),
                        "entries_consumed": int(r["hypotheses"]), "rounds": int(r["rounds"])}}
        cloud = torch.from_numpy(synth.scene(1_000_000, seed=42)).to("cuda")
        torch.cuda.synchronize()
        tests = 0
        for _ in range(a.yardstick):
            r = ctx.sac_segment(cloud, labels=False, distance_threshold=0.2, max_iterations=1000)
            tests += entries_evaluated(r["rounds"], 1000) * len(cloud)
        out["sac"] = {"points": int(len(cloud)), "plane_tests": int(tests), "skipped": int(r["skipped"]),
                      "entries_consumed": int(r["hypotheses"]), "rounds": int(r["rounds"])}
        ctx.close()
        print(json.dumps(out))
        return
    out = {"metric": "wm_corr_ransac ms per call, inputs in device memory (median of calls)", "calls": a.calls,
           "inlier_threshold": thr, "max_iterations": 1000}
    for m in [int(x) for x in a.sizes.split(",") if x]:
        for share in [float(x) for x in a.shares.split(",") if x]:
            args = tuple(torch.from_numpy(x).to("cuda") for x in planted(m, share, thr, m % 1000 + int(share * 10)))
            torch.cuda.synchronize()
            for refine in (0, 1):
                out["m_%d_inliers_%g_refine_%d" % (m, share, refine)] = timed(ctx, args, a.calls, a.warmup, max_iterations=1000,
                                                                             refine_model=refine)
            del args
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
