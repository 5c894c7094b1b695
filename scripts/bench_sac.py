"""wm_sac_segment timing: device milliseconds per call (wm_sac_stats.kernel_ms: HIP events from the cloud's packing to
the last output, the rounds' fetches and the refit's included) and host milliseconds per call (clock around a call,
which ends in its own synchronise), with the cloud resident in device memory, on synth.scene(1M) and on the 64-ring
synth.scene_rings(2M) scan, at thresholds 0.05 m and 0.2 m and max_iterations 50 and 1000, PCL's other defaults, seed 0.
Every figure is the median of --calls calls after --warmup, with the fastest and slowest call beside it; the loop's
counters (iterations, rounds, entries) say how much work a call was.  The same 2M scan through wm_ground_segment (host
milliseconds per call, as scripts/bench_ground.py measures it: compare with host_ms) is the yardstick beside it.
Prints one JSON line.

--round R[,R...]   again under option sac_round = R.
--yardstick N      N calls per cloud of wm_sac_segment at threshold 0.2 m, max_iterations 1000, and N of
                   wm_ground_segment on the 2M scan.  Meant to run under `rocprofv3 --kernel-trace --stats`, whose
                   per-kernel times give k_sac_count's plane tests per second: the JSON line carries the number of
                   plane tests (valid entries evaluated x points) the N calls made per cloud; nothing else is timed.
--batch S[,S...]   instead of the above, the key "batch": wm_sac_segment_batch over S scans against the same S scans
                   through wm_sac_segment one after the other on the same context, the two alternating; host ms PER
                   SCAN (clock around calls that end in their own synchronise), the median of --rounds rounds, one entry
                   per repeat (--repeats: their range is the run-to-run spread).  Device input, no labels; threshold
                   0.05 m / max_iterations 50 and 0.2 m / 1000; the scans: 4 000 ... 20 000 points each, every 50th
                   point of synth.scene(1M) from offset k.  --loop-only times the loop of single calls alone (what a
                   library without the batch entry can run: the yardstick is that loop on the parent commit's library).
                   --round R[,R...] adds the batch and the loop under option sac_round = R."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, cloud, calls, warmup, **kw):
    for _ in range(warmup):
        ctx.sac_segment(cloud, labels=False, **kw)
    dev, host = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = ctx.sac_segment(cloud, labels=False, **kw)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(r["kernel_ms"])
    return {"device_ms": round(float(np.median(dev)), 4), "device_ms_min_max": [round(float(min(dev)), 4), round(float(max(dev)), 4)],
            "host_ms": round(float(np.median(host)), 4), "rc": int(r["rc"]), "iterations": int(r["iterations"]),
            "rounds": int(r["rounds"]), "entries": int(r["hypotheses"]), "inliers": int(r["n_out"]),
            "n_finite": int(r["n_finite"])}


def bench_batch(ctx, host, sizes, rounds, warmup, repeats, loop_only, round_sizes):
    import torch
    top = max(sizes)
    scans = [torch.from_numpy(np.ascontiguousarray(host[k % 50::50][:4000 + (k * 3000) % 16001])).to("cuda") for k in range(top)]
    settings = {"thr_0.05_it_50": dict(distance_threshold=0.05, max_iterations=50),
                "thr_0.2_it_1000": dict(distance_threshold=0.2, max_iterations=1000)}
    out = {"metric": "host ms per scan (median of rounds; one entry per repeat)", "rounds": rounds, "repeats": repeats,
           "points_per_scan": {"S%d" % S_: int(np.mean([len(s) for s in scans[:S_]])) for S_ in sizes}}
    torch.cuda.synchronize()
    for R in [256] + [r for r in round_sizes if r != 256]:
        ctx.set_option("sac_round", R)
        for _ in range(repeats):  # the whole measurement, again
            for sname, params in settings.items():
                for S_ in sizes:
                    clouds = scans[:S_]
                    for _ in range(max(warmup // S_, 2)):
                        for c in clouds:
                            ctx.sac_segment(c, labels=False, **params)
                        if not loop_only:
                            ctx.sac_segment_batch(clouds, labels=False, **params)
                    tl, tb = [], []
                    for _ in range(rounds):
                        t0 = time.perf_counter()
                        for c in clouds:
                            r = ctx.sac_segment(c, labels=False, **params)
                        t1 = time.perf_counter()
                        if not loop_only:
                            b = ctx.sac_segment_batch(clouds, labels=False, **params)
                        t2 = time.perf_counter()
                        tl.append((t1 - t0) * 1e3 / S_)
                        tb.append((t2 - t1) * 1e3 / S_)
                    key = "%s_S%d" % (sname, S_) + ("" if R == 256 else "_round%d" % R)
                    cell = out.setdefault(key, {"loop_ms_per_scan": [], "batch_ms_per_scan": []})
                    cell["loop_ms_per_scan"].append(round(float(np.median(tl)), 4))
                    cell["last_scan_rounds"] = int(r["rounds"])
                    if not loop_only:
                        cell["batch_ms_per_scan"].append(round(float(np.median(tb)), 4))
                        cell["batch_rounds"] = int(max(g["rounds"] for g in b))
    ctx.set_option("sac_round", 256)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="", help="S[,S...]: time wm_sac_segment_batch against a loop of single calls")
    ap.add_argument("--rounds", type=int, default=30, help="rounds of a --batch cell")
    ap.add_argument("--repeats", type=int, default=3, help="repeats of the whole --batch measurement")
    ap.add_argument("--loop-only", action="store_true", help="with --batch: only the loop of single calls")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clouds", default="scene_1m,rings_2m")
    ap.add_argument("--thresholds", default="0.05,0.2")
    ap.add_argument("--max-iterations", default="50,1000")
    ap.add_argument("--round", default="", help="R[,R...]: again under option sac_round = R")
    ap.add_argument("--yardstick", type=int, default=0, help="calls of sac_segment and ground_segment, for a kernel trace")
    a = ap.parse_args()
    thresholds = [float(x) for x in a.thresholds.split(",") if x]
    max_its = [int(x) for x in a.max_iterations.split(",") if x]
    import torch
    from libwave_amd import capi, synth
    ctx = capi.Context(0)
    sizes = [int(x) for x in a.batch.split(",") if x]
    if sizes:
        out = {"batch": bench_batch(ctx, synth.scene(1_000_000, seed=42), sizes, a.rounds, a.warmup, a.repeats, a.loop_only,
                                    [int(x) for x in a.round.split(",") if x])}
        ctx.close()
        print(json.dumps(out))
        return
    make = {"scene_1m": lambda: torch.from_numpy(synth.scene(1_000_000, seed=42)).to("cuda"),
            "rings_2m": lambda: torch.from_numpy(synth.scene_rings(2_000_000, seed=42)).to("cuda")}
    out = {"metric": "wm_sac_segment ms per call, cloud in device memory (median of calls)", "calls": a.calls}
    for name in [c for c in a.clouds.split(",") if c]:
        cloud = make[name]()
        torch.cuda.synchronize()
        row = {"points": int(len(cloud))}
        if a.yardstick:
            tests = 0
            for _ in range(a.yardstick):
                r = ctx.sac_segment(cloud, labels=False, distance_threshold=0.2, max_iterations=1000)
                # a round holds min(256, max_iterations + 1 - it) entries: exact while no entry is skipped (see "skipped")
                tests += min(r["rounds"] * 256, 1001) * len(cloud)
            row["yardstick_calls"] = a.yardstick
            row["plane_tests"] = int(tests)
            row["skipped"] = int(r["skipped"])
            row["entries_consumed"] = int(r["hypotheses"])
            row["rounds"] = int(r["rounds"])
            if name == "rings_2m":
                for _ in range(a.yardstick):
                    ctx.ground_segment(cloud)
        else:
            for thr in thresholds:
                for mi in max_its:
                    row["thr_%g_it_%d" % (thr, mi)] = timed(ctx, cloud, a.calls, a.warmup, distance_threshold=thr, max_iterations=mi)
            for R in [int(x) for x in a.round.split(",") if x]:
                ctx.set_option("sac_round", R)
                for thr in thresholds:
                    for mi in max_its:
                        row["thr_%g_it_%d_round%d" % (thr, mi, R)] = timed(ctx, cloud, a.calls, a.warmup, distance_threshold=thr,
                                                                          max_iterations=mi)
                ctx.set_option("sac_round", 256)
            if name == "rings_2m":
                ms = []
                for k in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    ctx.ground_segment(cloud)
                    if k >= a.warmup:
                        ms.append((time.perf_counter() - t0) * 1e3)
                row["ground_segment_host_ms"] = round(float(np.median(ms)), 4)
        out[name] = row
        del cloud
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
