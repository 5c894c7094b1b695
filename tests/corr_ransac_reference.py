"""The checker of wm_corr_ransac (include/wavematch.h, "pose from correspondences"): PCL 1.8's
CorrespondenceRejectorSampleConsensus as the header restates it, in numpy.  The stream is sac_reference's, the count is
float32 operation by operation, the loop is the header's in literal form.  The hypothesis is stated twice:

  hypothesis_lib   through wm.corr_hypothesis, the library's HOST evaluation of the rule (no device): what the device
                   must equal bit for bit;
  hypothesis_svd   a float64 numpy.linalg.svd restatement of Umeyama, with no project code in it.

tests/test_corr_ransac_reference_cpu.py holds the first to the second."""
import math
import sys

import numpy as np

import sac_reference as SR

NONE, INLIER, OUTLIER = 0, 1, 2
OK, NOT_CONVERGED = 0, 1
F = np.float32
U = 2.0 ** -23


# ------------------------------------------------------------------ the pairs
def pairs_of(src, tgt, match_idx, query_idx=None):
    """-> (P float32 [mv, 3], Q float32 [mv, 3], e int [mv]): the valid entries, ascending by e"""
    src = np.asarray(src, F)[:, :3]
    tgt = np.asarray(tgt, F)[:, :3]
    mi = np.asarray(match_idx, np.int64)
    qi = np.arange(len(mi), dtype=np.int64) if query_idx is None else np.asarray(query_idx, np.int64)
    ok = (qi >= 0) & (qi < len(src)) & (mi >= 0) & (mi < len(tgt))
    e = np.nonzero(ok)[0]
    fin = np.isfinite(src[qi[e]]).all(1) & np.isfinite(tgt[mi[e]]).all(1)
    e = e[fin]
    return np.ascontiguousarray(src[qi[e]]), np.ascontiguousarray(tgt[mi[e]]), e


# ------------------------------------------------------------------ thresholds
def thr2_f(thr):
    """the smallest float32 not below thr^2 (float64)"""
    return SR.thr_f(float(thr) * float(thr))


def min_d2_given(d):
    return F(float(d) * float(d))


def min_d2_auto(P):
    """((sqrt l0 + sqrt l1 + sqrt l2) / 3)^2 of the covariance of P normalised by its size, the eigenvalues clamped at 0"""
    with np.errstate(all="ignore"):
        D = P.astype(np.float64) - P[0].astype(np.float64)
        mean = D.sum(0) / len(D)
        Cm = D.T @ D / len(D) - np.outer(mean, mean)
    if not np.isfinite(Cm).all():
        return F(0)
    lam = np.maximum(np.linalg.eigvalsh(Cm), 0.0)
    r = np.sqrt(lam).sum() / 3.0
    out = F(r * r)
    return out if np.isfinite(out) else F(0)


# ------------------------------------------------------------------ the sample test
def _d2(a, b):
    d = b - a
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def sample_good(p, min_d2):
    """p float32 [3, 3]: the sample's source points"""
    p = np.asarray(p, F)
    min_d2 = F(min_d2)
    with np.errstate(all="ignore"):
        if not (_d2(p[0], p[1]) > min_d2 and _d2(p[0], p[2]) > min_d2 and _d2(p[1], p[2]) > min_d2):
            return False
        u, v = p[1] - p[0], p[2] - p[0]
        cx = u[1] * v[2] - u[2] * v[1]
        cy = u[2] * v[0] - u[0] * v[2]
        cz = u[0] * v[1] - u[1] * v[0]
        s = (cx * cx + cy * cy) + cz * cz
        return bool(np.isfinite(s) and s > 0)


# ------------------------------------------------------------------ the hypothesis, twice
def hypothesis_lib(p, q, min_d2):
    """-> T float32 [3, 4] or None (skipped): wm.corr_hypothesis"""
    from libwave_amd import capi as wm
    flag, T = wm.corr_hypothesis(p, q, min_d2)
    return T if flag else None


def umeyama64(P, Q):
    """Umeyama without scaling in float64 -> [4, 4]: Q ~ R P + t"""
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    pm, qm = P.mean(0), Q.mean(0)
    sigma = (Q - qm).T @ (P - pm) / len(P)
    Um, S, Vt = np.linalg.svd(sigma)
    d = 1.0 if np.linalg.det(Um) * np.linalg.det(Vt) > 0 else -1.0
    R = Um @ np.diag([1.0, 1.0, d]) @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = qm - R @ pm
    return T, S


def hypothesis_svd(p, q, min_d2):
    """-> (T float32 [3, 4], singular values) or None: the sample test, then umeyama64 rounded to float32"""
    if not sample_good(p, min_d2):
        return None
    T, S = umeyama64(p, q)
    Tf = T[:3].astype(F)
    if not np.isfinite(Tf).all():
        return None
    return Tf, S


# ------------------------------------------------------------------ the count
def inliers(P, Q, T, th2):
    """bool [mv]: float32, every operation rounded, nothing fused"""
    T = np.asarray(T, F)
    with np.errstate(all="ignore"):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        dx = (((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]) - Q[:, 0]
        dy = (((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]) - Q[:, 1]
        dz = (((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]) - Q[:, 2]
        return ((dx * dx + dy * dy) + dz * dz) < th2


# ------------------------------------------------------------------ the loop
def walk_counts(flags, counts, n, max_it=1000, prob=0.99):
    """The header's loop over a given stream of (flag, count) entries: flag 0 skipped, 1 valid."""
    it = skipped = j = 0
    k, best, best_j = 1.0, -1, -1
    eps = sys.float_info.epsilon
    log_p = math.log(1.0 - prob)
    max_skip = 10 * max_it
    while it < k and skipped < max_skip:
        flag, count = flags[j], counts[j]
        j += 1
        if not flag:
            skipped += 1
            continue
        if count > best:
            best, best_j = int(count), j - 1
            k = log_p / math.log(min(1.0 - eps, max(eps, 1.0 - (count / n) ** 3)))
        it += 1
        if it > max_it:
            break
    return dict(iterations=it, skipped=skipped, hypotheses=j, best_hypothesis=best_j, n_inliers_model=max(best, 0))


def run_literal(P, Q, thr, max_it=1000, prob=0.99, seed=0, min_d2=0.0, hyp=hypothesis_lib):
    """One hypothesis at a time, the loop exactly as the header writes it, over the pairs (P, Q)."""
    n = len(P)
    it = skipped = j = 0
    k, best, best_j, best_T = 1.0, -1, -1, None
    if n >= 3:
        th2 = thr2_f(thr)
        eps = sys.float_info.epsilon
        log_p = math.log(1.0 - prob)
        max_skip = 10 * max_it
        while it < k and skipped < max_skip:
            i = list(SR.sample(seed, j, n))
            T = hyp(P[i], Q[i], min_d2)
            j += 1
            if T is None:
                skipped += 1
                continue
            if isinstance(T, tuple):
                T = T[0]
            count = int(inliers(P, Q, T, th2).sum())
            if count > best:
                best, best_j, best_T = count, j - 1, T
                k = log_p / math.log(min(1.0 - eps, max(eps, 1.0 - (count / n) ** 3)))
            it += 1
            if it > max_it:
                break
    return dict(status=OK if best_j >= 0 else NOT_CONVERGED, iterations=it, skipped=skipped, hypotheses=j,
                best_hypothesis=best_j, n_inliers_model=max(best, 0), model=best_T)


# ------------------------------------------------------------------ the whole call
def select(P, Q, e, m, T, thr):
    """-> (the kept entries ascending int32, labels uint8 [m]) of the transform's float32 rounding"""
    inl = inliers(P, Q, np.asarray(T)[:3].astype(F), thr2_f(thr))
    labels = np.zeros(m, np.uint8)
    labels[e] = np.where(inl, INLIER, OUTLIER)
    return e[inl].astype(np.int32), labels


def solve(src, tgt, match_idx, query_idx=None, thr=0.05, max_it=1000, prob=0.99, seed=0, min_sample_distance=-1.0,
          refine=False, min_d2=None, hyp=hypothesis_lib):
    """The whole call.  min_d2: the bound to apply (e.g. the device's own), else from min_sample_distance."""
    P, Q, e = pairs_of(src, tgt, match_idx, query_idx)
    m = len(match_idx)
    if min_d2 is None:
        min_d2 = (min_d2_auto(P) if len(P) else F(0)) if min_sample_distance < 0 else min_d2_given(min_sample_distance)
    out = run_literal(P, Q, thr, max_it, prob, seed, min_d2, hyp)
    out.update(n_valid=len(P), min_d2=F(min_d2), T=None, inliers=np.zeros(0, np.int32), labels=None, refined=0)
    if out["status"] != OK:
        return out
    T = np.eye(4)
    T[:3] = out["model"].astype(np.float64)
    if refine and out["n_inliers_model"] >= 3:
        inl = inliers(P, Q, out["model"], thr2_f(thr))
        T, _ = umeyama64(P[inl].astype(np.float64) - P[inl][0].astype(np.float64),
                         Q[inl].astype(np.float64) - Q[inl][0].astype(np.float64))
        T[:3, 3] = Q[inl][0].astype(np.float64) + T[:3, 3] - T[:3, :3] @ P[inl][0].astype(np.float64)
        out["refined"] = 1
    out["T"] = T
    out["inliers"], out["labels"] = select(P, Q, e, m, T, thr)
    return out


# ------------------------------------------------------------------ inputs
def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def planted(m, share, thr, seed, box=10.0, angle=math.radians(40.0), axis=(1, 2, 3), shift=2.0, offset=0.0):
    """m pairs, entry e pairs source e with target e: a `share` of them inliers of a rotation about `axis` with `shift`
    metres of translation and noise of norm <= thr / 4, the rest uniform outliers in the box.
    -> (src, tgt float32 [m, 3], match_idx int32 [m], planted bool [m], T float64 [4, 4])"""
    rng = np.random.default_rng(seed)
    R = rotation(axis, angle)
    t = shift * np.array([2.0, -1.0, 2.0]) / 3.0
    src = rng.uniform(-box, box, (m, 3))
    tgt = rng.uniform(-box, box, (m, 3))
    good = rng.permutation(m) < int(round(share * m))
    noise = rng.normal(size=(m, 3))
    noise *= (rng.uniform(0, thr / 4, m) / np.linalg.norm(noise, axis=1))[:, None]
    tgt[good] = (src[good] @ R.T + t + noise[good])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    if offset:
        src = src + offset
        tgt = tgt + offset
        T[:3, 3] = t + offset - R @ np.full(3, offset)
    return (np.ascontiguousarray(src, F), np.ascontiguousarray(tgt, F), np.arange(m, dtype=np.int32), good, T)
