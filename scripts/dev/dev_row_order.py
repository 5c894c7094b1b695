"""Developer: the work of the early searches, for comparing visiting orders of a box's rows between two trees.
Per iteration 0-5 of the 1M bench pair and of the 64-ring pair: row chunks and candidate trips per query
(wm_debug_cost_log: the mechanism, no clocks involved), what a wavefront pays for them (its slowest lane's chunks, its
pooled trips / 64), and the same split by the number of passes a query needed.  Between a tree that walks a box
from its corner and one that walks it nearest-first the difference IS the over-scan: chunks and trips spent on rows
farther away than the neighbour finally found (profiles/row_order_experiments.md).  Also the seed radius over the
distance found (r_seed / h) of the seeded iterations, from the matches and poses of consecutive aligns.  The checksum of
the correspondences is printed for comparing the trees' results."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from libwave_amd import capi, synth

N = 1_000_000
ITERS = 6


def costs(d_ref, d_tgt):
    ctx = capi.Context(0)
    ctx.set_source(d_ref)
    ctx.set_target(d_tgt)
    n = ctx.sizes()[0]
    ctx.cost_log_arm(ITERS)
    r = ctx.icp_align(max_corr=3.0, force_iterations=ITERS, nn_method=capi.WM_NN_GRID, profile=0, carry_state=0)
    log = ctx.cost_log_fetch(ITERS, n)
    corr = ctx.correspondences()
    ctx.close()
    return r, log, corr, n


def seed_ratio(ref, tgt, d_ref, d_tgt):
    """r_seed / h per seeded iteration: the match of search k-1, re-measured under the pose search k runs at, over the
    distance search k finds (align(K) leaves search K-1's matches, made under align(K-1)'s pose)."""
    res = []
    for K in range(1, ITERS + 2):
        ctx = capi.Context(0)
        ctx.set_source(d_ref)
        ctx.set_target(d_tgt)
        r = ctx.icp_align(max_corr=3.0, force_iterations=K, nn_method=capi.WM_NN_GRID, profile=0, carry_state=0)
        res.append((r["T"], ctx.correspondences()))
        ctx.close()
    for k in range(1, ITERS):
        (idx_prev, _), T_k, (idx_k, d2_k) = res[k - 1][1], res[k - 1][0], res[k][1]
        ok = (idx_prev >= 0) & (idx_k >= 0) & (d2_k > 0)
        moved = ref[ok, :3].astype(np.float64) @ T_k[:3, :3].T + T_k[:3, 3]
        r_seed = np.linalg.norm(moved - tgt[idx_prev[ok], :3], axis=1)
        q = np.quantile(r_seed / np.sqrt(d2_k[ok].astype(np.float64)), [0.25, 0.5, 0.75, 0.9, 0.99])
        print("  it %d: r_seed / h quantiles 25/50/75/90/99 %%: %s   match kept: %.1f %%" % (
            k, np.round(q, 2), 100.0 * (idx_prev[ok] == idx_k[ok]).mean()), flush=True)


for pattern in ("default", "rings"):
    kw = {} if pattern == "default" else {"pattern": pattern}
    ref, tgt, _ = synth.pair(N, seed=42, **kw)
    d_ref, d_tgt = torch.from_numpy(ref).cuda(), torch.from_numpy(tgt).cuda()
    print("== %s pair" % pattern, flush=True)
    seed_ratio(ref, tgt, d_ref, d_tgt)
    r, log, corr, n = costs(d_ref, d_tgt)
    print("-- cell %.3f m; correspondences: sum of indices %d, of d2 bits %d" % (
        r["grid_cell"], corr[0].astype(np.int64).sum(), corr[1].view(np.uint32).astype(np.int64).sum()), flush=True)
    for it in range(len(log)):
        c = log[it]
        trips, chunks = (c & 0xFFFF).astype(np.int64), ((c >> 16) & 0xFF).astype(np.int64)
        passes = ((c >> 24) & 0xF).astype(np.int64)  # (bits 28-30: probe rungs)
        w = np.pad(chunks, (0, (-n) % 64)).reshape(-1, 64)
        t = np.pad(trips, (0, (-n) % 64)).reshape(-1, 64)
        print("  it %d: chunks/query %.2f, trips/query %.2f | per wave: max-lane chunks %.1f, trips/64 %.1f | heavy %d" % (
            it, chunks.mean(), trips.mean(), w.max(1).mean(), t.sum(1).mean() / 64, (c >> 31).sum()), flush=True)
        for p in range(1, 7):
            m = passes == p
            if m.sum() > n // 1000:
                print("        passes=%d: %5.1f %% of queries, chunks mean %.1f, trips mean %.1f" % (
                    p, 100.0 * m.mean(), chunks[m].mean(), trips[m].mean()), flush=True)
