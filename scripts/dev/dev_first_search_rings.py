"""The 1M 64-ring pair through the C ABI: registration time and the first (unseeded) search of it.
usage: dev_first_search_rings.py [runs] [tree]  -- prints one line per run; the library is the one built in `tree`
(default: the tree this script lies in), so two trees are compared by running the script once per tree, alternately."""
import os, sys, time
sys.path.insert(0, os.path.abspath(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")))
import numpy as np
import torch
from libwave_amd import capi, synth

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
ref, tgt, T_gt = synth.pair(1_000_000, seed=42, pattern="rings")
d_ref, d_tgt = torch.from_numpy(ref).cuda(), torch.from_numpy(tgt).cuda()
ctx = capi.Context(0)


def step(profile=0):
    ctx.set_source(d_ref)
    ctx.set_target(d_tgt)
    return ctx.icp_align(max_corr=3.0, force_iterations=50, nn_method=capi.WM_NN_GRID, profile=profile, carry_state=0)


for _ in range(3):
    step()
for k in range(runs):
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        r = step()
        ts.append((time.perf_counter() - t0) * 1e3)
    step(1)
    it = ctx.iteration_times() * 1e3
    print("rings run %d: %.4f ms per registration (median of 20, min %.4f); search of iteration 0 %.1f us, iterations 1-24 %.1f us; "
          "cert launches %d" % (k, np.median(ts), min(ts), it[0], it[1:25].sum(), r["cert_launches"]), flush=True)
ctx.close()
