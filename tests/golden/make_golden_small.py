#!/usr/bin/env python3
"""Record tests/golden/small_icp_bits.json -- what wm_icp_batch_match (csrc/wm_small.hip, wm_batch.hip) and the one-pair
path's statistics and LUMold kernels (wm_icp.hip, wm_info.hip) return, bit for bit, on the library as it stands (needs
the GPU).  tests/test_batch_gpu.py holds the small path to the oracle and to the one-pair path within 1e-7 ... 1e-9; it
does not pin the bits of T and info, which depend on which chunk row a query's terms land in, on the fixed order the
rows are added in and on the float and double forms of every term.  tests/test_small_pinned_gpu.py holds the library to
this record.

The inputs (max_corr 3.0 throughout; clouds of synth.pair(..., "resample"), cut to size by a seeded choice), each the
smallest that reaches a branch of the kernel:
  target in LDS (<= 10 000 points), SVD and GN6 with force_iterations=6 and info
    1  64 <- 64             one chunk, fifteen idle waves, the sort padded to 2 048
    2  1 100 <- 900         18 chunks for 16 waves (the ticket is drawn); n_tgt % 4 != 0 (the candidate loop reads sentinels)
                            (also with the default stopping rules, max_iter=100, with and without info)
    3  2 048 <- 1 000       the sort's padded size equals n_src
    4  16 385 <- 2 000      every 9th source point NaN: past the 2^14 sort window, non-finite queries inside the loop
    5  1 000 <- 10 000      all ten per-lane slots of the counting sort, LDS full
    6  3 000 <- 3 000       NaN and inf holes in both clouds
  edge inputs, max_iter=50 with info
    7  a flat cloud, z == 0 exactly, 500 points (GN6: its -px * pz terms are -0.0; and SVD)
    8  100 identical points
    9  a target 500 m away: nothing within max_corr
  target in HBM scratch, SVD and GN6 with force_iterations=6 and info
    10 1 100 <- 10 001      the smallest HBM target
    11 32 769 <- 10 001     holes in the source, past the 2^15 sort window
    12 20 000 <- 12 000     sorted here, would not be with the target in LDS
    13 500 <- 65 535        the 16-bit slot limit, 64 512 cells
  the voxel-filtered route (wm_batch.hip: presorted sources, prev_mse0 carried from scale to scale)
    14 3 000 <- 3 000 at res=0.25, multiscale_steps 0 and 2
  the one-pair path
    15 the pairs of 2 and 10: icp_match's T, icp_info LUMOLD and LUM, icp_stats_for in both modes, and an icp_match
       with trimmed rejection
Per item: rc, the float64 words (hex) of T, info, mse, prev_mse and grid_cell, iterations, state, n_corr, and the SHA-256
and length of both clouds.  The cycle counters in nn_ms / stats_ms / solve_ms / coarse_ms are not recorded.

    python tests/golden/make_golden_small.py [--lib PATH] [--out FILE]    # rewrites small_icp_bits.json (GPU)
    python tests/golden/make_golden_small.py --check-oracle               # the conditions on the inputs (CPU)
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "small_icp_bits.json")
SVD, GN6 = 0, 1  # WM_ICP_SVD, WM_ICP_GN6
FORCED = [("svd-force6", dict(force_iterations=6, mode=SVD)), ("gn6-force6", dict(force_iterations=6, mode=GN6))]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _words(a):
    return None if a is None else ["%016x" % int(v) for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)]


def _cut(cloud, n, seed):
    """n points of `cloud`, in its order, by a seeded choice (the overlap of a pair stays)"""
    if n == len(cloud):
        return cloud
    keep = np.sort(np.random.default_rng(seed).choice(len(cloud), n, replace=False))
    return np.ascontiguousarray(cloud[keep])


def _pair(n_src, n_tgt, seed):
    from libwave_amd import synth
    ref, tgt, _ = synth.pair(max(n_src, n_tgt), seed=seed, mode="resample")
    return _cut(ref, n_src, seed + 1), _cut(tgt, n_tgt, seed + 2)


_CLOUDS = None


def clouds():
    """-> {input number: (source, target)}, float32 [n, 3]"""
    global _CLOUDS
    if _CLOUDS is not None:
        return _CLOUDS
    c = {}
    c[1] = _pair(64, 64, 401)
    c[2] = _pair(1100, 900, 402)
    c[3] = _pair(2048, 1000, 403)
    s, t = _pair(16385, 2000, 404)
    s = s.copy()
    s[::9, 2] = np.nan
    c[4] = (s, t)
    c[5] = _pair(1000, 10000, 405)
    s, t = _pair(3000, 3000, 406)
    s, t = s.copy(), t.copy()
    s[::7, 1] = np.nan
    s[5::31, 0] = np.inf
    t[::5, 0] = np.inf
    t[3::17, 2] = np.nan
    c[6] = (s, t)
    rng = np.random.default_rng(407)
    flat = np.zeros((500, 3), np.float32)
    flat[:, :2] = rng.uniform(-5, 5, (500, 2))
    c[7] = (flat, (flat + np.array([0.01, 0.01, 0.0], np.float32)).astype(np.float32))
    same = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (100, 1))
    c[8] = (same, same.copy())
    s, t = _pair(600, 600, 409)
    c[9] = (s, (t + np.array([500.0, 0, 0], np.float32)).astype(np.float32))
    c[10] = _pair(1100, 10001, 410)
    s, t = _pair(32769, 10001, 411)
    s = s.copy()
    s[::9, 2] = np.nan
    s[4::13, 0] = np.inf
    c[11] = (s, t)
    c[12] = _pair(20000, 12000, 412)
    c[13] = _pair(500, 65535, 413)
    c[14] = _pair(3000, 3000, 414)
    for s, t in c.values():
        s.setflags(write=False)
        t.setflags(write=False)
    _CLOUDS = c
    return c


def inputs():
    """-> [(id of the parameter set, keywords of Context.icp_batch_match, [(id of the item, source, target), ...])], the
    order of the record.  The items of one set go in one call (LDS and HBM targets mixed) or in a call each."""
    c = clouds()
    out = []
    for name, kw in FORCED:
        out.append((name, dict(kw, with_info=True, max_corr=3.0), [("%d/%s" % (k, name),) + c[k] for k in (1, 2, 3, 4, 5, 6, 10, 11, 12, 13)]))
    out.append(("default-info", dict(with_info=True, max_corr=3.0, max_iter=100), [("2/default-info",) + c[2]]))
    out.append(("default-noinfo", dict(with_info=False, max_corr=3.0, max_iter=100), [("2/default-noinfo",) + c[2]]))
    out.append(("edge-gn6", dict(with_info=True, max_corr=3.0, max_iter=50, mode=GN6), [("7/edge-gn6",) + c[7]]))
    out.append(("edge-svd", dict(with_info=True, max_corr=3.0, max_iter=50, mode=SVD),
                [("%d/edge-svd" % k,) + c[k] for k in (7, 8, 9)]))
    for steps in (0, 2):
        name = "res0.25-steps%d" % steps
        out.append((name, dict(with_info=True, max_corr=3.0, max_iter=100, res=0.25, multiscale_steps=steps),
                    [("14/%s" % name,) + c[14]]))
    return out


def one_pair_inputs():
    """-> [(id, source, target)] of input 15"""
    c = clouds()
    return [("15/pair-of-2",) + c[2], ("15/pair-of-10",) + c[10]]


def digest(got):
    """what the record keeps of one dict of Context.icp_batch_match (or of icp_match)"""
    return dict(rc=int(got["rc"]), T=_words(got["T"]), info=_words(got.get("info")), iterations=int(got["iterations"]),
                state=str(got["state"]), n_corr=int(got["n_corr"]), mse=_words(got["mse"]), prev_mse=_words(got["prev_mse"]),
                grid_cell=_words(got["grid_cell"]))


def clouds_digest(src, tgt):
    return dict(src_sha256=_sha(src), n_src=len(src), tgt_sha256=_sha(tgt), n_tgt=len(tgt))


def one_pair(ctx, src, tgt):
    """input 15 on a context: -> what the record keeps"""
    from libwave_amd import capi
    m = ctx.icp_match(src, tgt, res=-1.0, max_corr=3.0, max_iter=100, carry_state=0)
    rec = dict(match=digest(m))
    for name, method in (("lumold", capi.WM_INFO_LUMOLD), ("lum", capi.WM_INFO_LUM)):
        rc, info, deg = ctx.icp_info(method, max_corr=3.0)
        rec[name] = dict(rc=int(rc), info=_words(info), degenerate=bool(deg))
    T = m["T"] if m["T"] is not None else np.eye(4)
    rec["stats_svd"] = _words(ctx.icp_stats_for(T, capi.WM_ICP_SVD))
    rec["stats_gn6"] = _words(ctx.icp_stats_for(T, capi.WM_ICP_GN6))
    rec["match_trimmed"] = digest(ctx.icp_match(src, tgt, res=-1.0, max_corr=3.0, max_iter=100, carry_state=0,
                                                reject=capi.WM_REJECT_TRIMMED))
    return rec


def load():
    with open(PATH) as f:
        return json.load(f)


def _finite(a):
    return np.ascontiguousarray(a[np.isfinite(a).all(1)])


def check_oracle():
    """the conditions on the inputs, on the CPU: every input but 7-9 gives the oracle rc == 0 and at least 3
    correspondences; the forced ones run their 6 iterations; input 2 converges under the default rules before 100"""
    from oracle import oracle_py as O
    for name, kw, items in inputs():
        for what, s, t in items:
            k = int(what.split("/")[0])
            if k in (7, 8, 9):
                continue
            s, t = _finite(s), _finite(t)
            if "res" in kw:
                m = O.IcpMatch(s, t, res=kw["res"], multiscale_steps=kw["multiscale_steps"], incremental_float=0, max_corr=3.0,
                               max_iter=kw["max_iter"])
                rc, n_corr, it = m.rc, m.r.n_corr, m.r.iterations
            else:
                okw = {k2: v for k2, v in kw.items() if k2 in ("force_iterations", "max_iter", "mode")}
                r = O.icp_align(s, t, max_corr=3.0, incremental_float=0, **okw)
                rc, n_corr, it = r["rc"], r["n_corr"], r["iterations"]
                if "force_iterations" in kw:
                    assert it == 6, (what, it)
                else:
                    assert r["converged"] and it < 100, (what, it)
            assert rc == 0 and n_corr >= 3, (what, rc, n_corr)
            print("%-28s rc %d  iterations %3d  n_corr %d" % (what, rc, it, n_corr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="", help="the library to record (default: the tree's)")
    ap.add_argument("--out", default=PATH)
    ap.add_argument("--check-oracle", action="store_true", help="check the conditions on the inputs with the oracle (CPU) and stop")
    a = ap.parse_args()
    if a.check_oracle:
        check_oracle()
        return
    from libwave_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    ctx = capi.Context(0)
    rec = {}
    for name, kw, items in inputs():
        got = ctx.icp_batch_match([(s, t) for _, s, t in items], **kw)
        for (what, s, t), g in zip(items, got):
            rec[what] = dict(digest(g), **clouds_digest(s, t))
            print(what, rec[what]["rc"], rec[what]["iterations"], rec[what]["state"], rec[what]["n_corr"])
    for what, s, t in one_pair_inputs():
        rec[what] = dict(one_pair(ctx, s, t), **clouds_digest(s, t))
        print(what, rec[what]["match"]["rc"], rec[what]["match"]["iterations"], rec[what]["match_trimmed"]["iterations"])
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
