"""Correspondence rejection in ICP restated in numpy: the checker of wm_icp_params.reject (libwave_amd/csrc/wm_reject.hip),
in the manner of plane_reference.py.  The contract is include/wavematch.h's (WM_REJECT_*), restated from PCL 1.8's
registration/impl/icp.hpp, correspondence_rejection_trimmed.cpp and correspondence_rejection_median_distance.cpp.

  select          the element of a 0-based rank of non-negative float32 values, by np.partition on their bit patterns
  threshold       the two rules exactly as the contract writes them, ties included -> (threshold as float32, all_kept):
                  FLT_MAX when the rule keeps everything whatever the distances, -1 when it rejects everything
  keep            d2 -> the kept mask under a threshold (bit patterns, signed: the device's comparison)
  align           the loop around oracle.KdTree: PR.transform_f32 for the pose, the rule on the matched pairs' float32
                  d2, oracle.umeyama (SVD) or PR.plane_sums / PR.step (PLANE) on the kept pairs, the stopping rules as
                  plane_reference.align states them, `margin` reported the same way; the kept pairs of the last iteration
  match           ICPMatcher::match()'s scales around align
"""
import numpy as np

import plane_reference as PR

NONE, TRIMMED, MEDIAN = 0, 1, 2
FLT_MAX = np.finfo(np.float32).max
SVD, GN6, PLANE = 0, 1, 2


def bits(d2):
    return np.ascontiguousarray(d2, np.float32).view(np.uint32)


def select(vals, rank):
    """the element of 0-based rank `rank` of the ascending non-negative float32 `vals` (they order as their bits do)"""
    b = bits(vals)
    assert 0 <= rank < len(b)
    return np.partition(b, rank)[rank:rank + 1].view(np.float32)[0]


def float_below(x):
    """the largest float32 whose double value does not exceed x (x >= 0); beyond FLT_MAX: FLT_MAX"""
    if not x < float(FLT_MAX):
        return FLT_MAX
    f = np.float32(x)
    if float(f) > x:
        f = np.nextafter(f, np.float32(-np.inf), dtype=np.float32)
    return np.float32(f)


def threshold(d2, reject, ratio=0.5, factor=1.0, min_corr=0):
    """d2: the matched pairs' float32 squared distances -> (threshold float32, all_kept)"""
    n = len(d2)
    if reject == NONE or n == 0:
        return FLT_MAX, True
    if reject == TRIMMED:
        k = max(int(np.floor(float(ratio) * float(n))), int(min_corr))
        if k >= n:
            return FLT_MAX, True
        if k == 0:
            return np.float32(-1.0), False
        return select(d2, k - 1), False  # the k-th smallest, 1-based; pairs tied with it are all kept
    assert reject == MEDIAN
    m = select(d2, n // 2)
    t = float_below(float(m) * float(factor))
    return t, bool(t == FLT_MAX)


def keep(d2, thr):
    """kept iff d2 <= threshold, as the device compares: the bit patterns as signed words"""
    return bits(d2).view(np.int32) <= np.float32(thr).reshape(1).view(np.int32)[0]


def reject_step(d2, reject, ratio=0.5, factor=1.0, min_corr=0):
    """-> dict(n_matched, n_kept, threshold, all_kept, kept) for one iteration's matched d2"""
    thr, allk = threshold(d2, reject, ratio, factor, min_corr)
    kept = keep(d2, thr)
    return dict(n_matched=len(d2), n_kept=int(kept.sum()), threshold=np.float32(thr), all_kept=allk, kept=kept)


def gn6_sums(p, q, d2):
    """the 32-slot GN layout of the point-to-point Gauss-Newton step (k_icp_stats<GN6> + expand_stats)"""
    p = np.asarray(p, np.float64)
    q = np.asarray(q, np.float64)
    st = np.zeros(32)
    st[0] = len(p)
    st[1] = np.asarray(d2, np.float64).sum()
    H = np.zeros((6, 6))
    g = np.zeros(6)
    I3 = np.eye(3)
    # J_i = [I | -[p_i]x], r_i = p_i - q_i
    sp = p.sum(0)
    H[:3, :3] = len(p) * I3
    K = np.array([[0, sp[2], -sp[1]], [-sp[2], 0, sp[0]], [sp[1], -sp[0], 0]])
    H[:3, 3:] = K
    H[3:, :3] = K.T
    pp = p.T @ p
    H[3:, 3:] = np.trace(pp) * I3 - pp
    r = p - q
    g[:3] = r.sum(0)
    g[3:] = np.cross(p, r).sum(0)
    st[2:23] = H[np.triu_indices(6)]
    st[23:29] = g
    return st


def align(oracle, src, tgt, reject=TRIMMED, ratio=0.5, factor=1.0, min_corr=0, mode=SVD, max_corr=3.0, max_iter=100,
          t_eps=1e-8, fit_eps=1e-2, k=PR.DEFAULT_K, tgt_normals=None, prev_mse=None):
    """-> dict(T, converged, iterations, state, n_corr, n_matched, threshold, mse, margin, kept_src, kept_tgt): n_corr and
    mse of the KEPT pairs (what PCL's estimation and criteria see), kept_src / kept_tgt the last iteration's kept pairs as
    indices into the given clouds."""
    src = np.ascontiguousarray(src, np.float32)
    tgt = np.ascontiguousarray(tgt, np.float32)
    smap = np.nonzero(np.isfinite(src).all(1))[0]
    src_f = src[smap]
    fin_t = np.isfinite(tgt).all(1)
    tmap = np.nonzero(fin_t)[0]
    if mode == PLANE and tgt_normals is None:
        tgt_normals = PR.normals(tgt, k)["normal"]
    tree = oracle.KdTree(tgt[fin_t])
    T = np.eye(4)
    prev = np.finfo(np.float64).max if prev_mse is None else prev_mse
    out = dict(T=None, converged=False, iterations=0, state=PR.CONV_NOT, n_corr=0, n_matched=0, threshold=np.float32(0), mse=0.0,
               margin=np.inf, kept_src=np.zeros(0, np.int64), kept_tgt=np.zeros(0, np.int64))
    it = 0
    while True:
        pf = PR.transform_f32(src_f, T)
        si, ti, d2 = PR.correspondences(tree, tgt, pf, max_corr)
        ti = tmap[ti]
        rj = reject_step(d2, reject, ratio, factor, min_corr)
        kp = rj["kept"]
        si, ti, d2k = si[kp], ti[kp], d2[kp]
        n = len(si)
        out["n_matched"], out["threshold"] = rj["n_matched"], rj["threshold"]
        out["n_corr"] = n
        out["kept_src"], out["kept_tgt"] = smap[si], ti
        out["mse"] = mse = float(d2k.astype(np.float64).sum() / n) if n else 0.0
        if n < 3:
            out["state"] = PR.CONV_NO_CORR
            break
        if mode == PLANE:
            st = PR.plane_sums(pf[si], tgt[ti], tgt_normals[ti], d2k)
            if PR.degenerate(st):
                out["state"] = PR.CONV_DEGENERATE
                break
            Tk = PR.step(st)
        elif mode == GN6:
            Tk = PR.step(gn6_sums(pf[si], tgt[ti], d2k))
        else:
            Tk = oracle.umeyama(pf[si], tgt[ti])
        T = Tk @ T
        it += 1
        out["iterations"] = it
        if it >= max_iter:
            out["state"], out["converged"] = PR.CONV_ITERATIONS, True
            break
        cos_angle = 0.5 * (Tk[0, 0] + Tk[1, 1] + Tk[2, 2] - 1.0)
        tsq = float(Tk[:3, 3] @ Tk[:3, 3])
        rel = abs(mse - prev) / prev
        out["margin"] = min(out["margin"], abs(rel - fit_eps) / fit_eps, abs(tsq - t_eps) / t_eps)
        state = PR.CONV_NOT
        if cos_angle >= 1.0 - t_eps and tsq <= t_eps:
            state = PR.CONV_TRANSFORM
        elif abs(mse - prev) < 1e-12:
            state = PR.CONV_ABS_MSE
        elif rel < fit_eps:
            state = PR.CONV_REL_MSE
        if state != PR.CONV_NOT:
            out["state"], out["converged"] = state, True
            break
        prev = mse
    out["prev_mse"] = prev
    out["T_last"] = T
    if out["converged"]:
        out["T"] = T
    return out


def match(oracle, ref, tgt, res=-1.0, multiscale_steps=0, max_corr=3.0, **kw):
    """ICPMatcher::match() (icp.cpp:75-133) with a rejector: every align of every scale rejects.
    -> (T or None, [align results per scale])."""
    runs = []
    if not res > 0:
        r = align(oracle, ref, tgt, max_corr=max_corr, **kw)
        return r["T"], [r]
    steps = max(int(multiscale_steps), 0)
    running = np.eye(4)
    prev = None
    for i in range(steps, -1, -1):
        leaf = np.float32(2.0 ** i * res)
        fr, ft = oracle.voxel_grid(ref, leaf), oracle.voxel_grid(tgt, leaf)
        mc = max_corr
        if steps > 0:
            fr = oracle.transform_cloud_d(fr, running)
            mc = 2.0 ** i * max_corr
        r = align(oracle, fr, ft, max_corr=mc, prev_mse=prev, **kw)
        runs.append(r)
        prev = r["prev_mse"]
        if not r["converged"]:
            return None, runs
        running = r["T"] @ running
    return running, runs


# ------------------------------------------------------------------ the issue's pairs
PARTIAL_T = ((0.5, -0.3, 0.05), (0.01, -0.02, 0.04))


def partial_pair(n=20000, cut=15.0):
    """synth.pair(n, resample) under PARTIAL_T; the source cut to x < cut in the reference frame, the target to the
    points whose pre-image has x > -cut: about 46 % overlap at cut = 15."""
    from libwave_amd import synth
    T = synth.make_T(*PARTIAL_T)
    ref, tgt, T_gt = synth.pair(n, mode="resample", T=T)
    pre = synth.transform_points(tgt, np.linalg.inv(T_gt))
    return ref[ref[:, 0] < cut].copy(), tgt[pre[:, 0] > -cut].copy(), T_gt


# crafted arrays of the select's tests: (name, function of n -> float32 values)
def crafted(n, seed=0):
    rng = np.random.default_rng(seed + n)
    u32 = lambda a: np.asarray(a, np.uint32).view(np.float32)  # noqa: E731
    base = np.uint32(0x3F000000)
    out = {
        "all equal": np.full(n, 0.37, np.float32),
        "zeros with denormals": u32(rng.integers(0, 4, n) * rng.integers(0, 2, n)),
        "bits 8-0": u32(base + rng.integers(0, 1 << 9, n).astype(np.uint32)),
        "bits 19-9": u32(base + (rng.integers(0, 1 << 11, n).astype(np.uint32) << np.uint32(9))),
        "exponent": u32((rng.integers(1, 255, n).astype(np.uint32) << np.uint32(23)) | np.uint32(0x00155555)),
        "uniform": rng.uniform(0, 9, n).astype(np.float32),
        "ascending": np.linspace(0, 9, n).astype(np.float32),
        "descending": np.linspace(9, 0, n).astype(np.float32),
    }
    return out


SELECT_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4097, 70001]


def select_ranks(n):
    return sorted({r for r in (0, 1, n // 2, n - 2, n - 1) if 0 <= r < n})
