"""A plain numpy statement of what GICP computes AFTER its covariances -- the pairs, the Mahalanobis matrices, both forms
of the objective and their gradients -- and the stress cases the kernels are held to, in the manner of ndt_reference.py.

  pairs          the 1-NN of the float-transformed source in the target, by brute force, with the strict distance gate
  mahalanobis    (C2 + R C1 R^T)^-1 by the adjugate in np.longdouble
  fdf_pcl        PCL's objective (OptimizationFunctorWithIndices::fdf): the residual through the FLOAT matrix of x,
                 widened, then r^T M r, sum M r and the rotation gradient
  fdf_statistics the function that the 74 sums of csrc/wm_gicp_quad.hpp represent, evaluated per pair: r = r0 + (T(x) - T0) z
  matrix_f       PCL's applyState on an identity base: Rz Ry Rx from float sines and cosines, float products

Every sum is a np.longdouble one (64 bits of mantissa: for a few thousand terms of one sign or of mixed signs, well
below a double's last bit), the rotation derivatives are products of the elementary rotations' derivatives -- not PCL's
table of nine entries per angle --, the inverse is not Eigen's cofactor order in double, and the 74 sums are never
formed.  Nothing of the library or of the oracle is imported: tests/test_gicp_reference_cpu.py holds this file to the C
oracle (oracle/gicp.c), tests/test_gicp_stress_gpu.py holds the kernels to both.

cases(): the clouds of knn_reference.shapes(), each against itself moved rigidly about its centroid, and cases cut from
`scene` -- see _build_cases."""
import math

import numpy as np

import knn_reference as KR

LD = np.longdouble
F32 = np.float32

# How far the oracle sits from this file over the cases and states of cases(), relative to |f| and to the largest
# gradient entry: the worst values that tests/test_gicp_reference_cpu.py prints (it fails if the oracle is more than
# twice as far), per objective and per group of (case, state) -- group_of() says which.
#   pcl_sums    both sides push every point through the same float matrix and differ in the order of their products
#               and in their sums (double-double there, long double here): last bits everywhere.
#   statistics  the oracle evaluates f from 74 sums, this file per pair.  Last bits as well, at the pairing pose, after
#               a translation-only step AND after a rotation step of 1e-4 rad, next to the origin as 55 km from
#               it (`far`): the rotation entries of D = T(x) - T0 (5e-9 to 1e-4) multiply sum M z z^T, which is
#               |z|^2 times the sums the translation entries meet, but that block is the correctly rounded sum of its terms: what it
#               contributes carries a relative 1e-16 of itself, and is of f's size at the most (csrc/wm_gicp_quad.hpp).
#               The rotated states keep groups of their own so that a change there shows.
#               (1e-8 appears if T(x) is formed by rounding the DOUBLE matrix of x: an ulp in two of its entries --
#               matrix_f forms it as applyState does.)
# (the measured worst rounded up to its second digit, and the case it comes from)
REF_VS_ORACLE_F = {
    "pcl_sums": {"near": 2.1e-16, "far": 2.0e-16},  # n63, utm_plane
    "statistics": {"near": 4.1e-16, "far": 2.0e-16, "near_rotated": 3.1e-16, "far_rotated": 1.7e-16},  # n10, utm_plane, n1025, utm
}
REF_VS_ORACLE_G = {
    "pcl_sums": {"near": 2.7e-16, "far": 4.1e-16},  # holes_both, utm
    "statistics": {"near": 2.9e-16, "far": 2.1e-16, "near_rotated": 7.9e-16, "far_rotated": 1.9e-16},  # three_pairs, utm, n255, utm_plane
}
OBJECTIVES = ("statistics", "pcl_sums")

MOTION_T = (0.05, -0.03, 0.02)  # the rigid motion that makes a case's target of its source: metres ...
MOTION_W = (0.001, -0.002, 0.003)  # ... and a rotation vector, radians, about the finite points' centroid
PAIR_X = (0.04, -0.02, 0.01, 0.0, 0.0, 0.0)  # the state the pairs are found under (exact floats' neighbours; utm*: see Case)
STEP_T = (0.01, 0.01, -0.01)  # the translation-only step of a centimetre ...
STEP_R = (1e-4, -1e-4, 1e-4)  # ... and the rotation added to it
MAX_CORR = 5.0  # PCL GICP's corr_dist_threshold_
SIZES = (10, 63, 64, 65, 255, 256, 257, 513, 1025)
FAR_AWAY = 1000.0  # "moved 1 km away"


# ------------------------------------------------------------------------------------------------- the transform
def matrix_f(x):
    """[4, 4] float32: applyState on an identity base -- Rz(x5) Ry(x4) Rx(x3) from the float sines and cosines of the
    float angles (correctly rounded: the double result rounded once), every product and sum rounded to float, left
    to right; the translation is x0..2 rounded to float"""
    f = F32
    (cphi, sphi), (cth, sth), (cpsi, spsi) = ((f(math.cos(float(f(x[k])))), f(math.sin(float(f(x[k]))))) for k in (3, 4, 5))
    T = np.zeros((4, 4), F32)
    T[0, :3] = [cpsi * cth, cpsi * sth * sphi - spsi * cphi, cpsi * sth * cphi + spsi * sphi]
    T[1, :3] = [spsi * cth, spsi * sth * sphi + cpsi * cphi, spsi * sth * cphi - cpsi * sphi]
    T[2, :3] = [-sth, cth * sphi, cth * cphi]
    T[:3, 3] = [f(x[0]), f(x[1]), f(x[2])]
    T[3, 3] = 1
    return T


def transform_f(T, pts):
    """((m00 x + m01 y) + m02 z) + m03, every operation rounded to float32"""
    T, p = np.asarray(T, F32), np.asarray(pts, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)
    assert out.dtype == F32
    return out


def _elementary(axis, angle, derivative=False):
    c, s = np.cos(LD(angle)), np.sin(LD(angle))
    if derivative:
        c, s = -s, c  # d/d(angle) of (cos, sin)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    E = np.zeros((3, 3), LD)
    if not derivative:
        E[axis, axis] = 1
    E[i, i], E[j, j], E[j, i], E[i, j] = c, c, s, -s
    return E


def rotation(x):
    """R = Rz(x5) Ry(x4) Rx(x3) and its derivatives by x3, x4, x5, in np.longdouble from the DOUBLE angles"""
    Rx, Ry, Rz = (_elementary(a, x[3 + a]) for a in range(3))
    dx, dy, dz = (_elementary(a, x[3 + a], True) for a in range(3))
    return Rz @ Ry @ Rx, [Rz @ Ry @ dx, Rz @ dy @ Rx, dz @ Ry @ Rx]


# ------------------------------------------------------------------------------------------------- the pairs
def pairs(src, tgt, T0f, max_corr, chunk=256):
    """-> (idx [n] int32, d2 [n] float32): for every source point, pushed through the float matrix T0f by transform_f,
    the target point with the smallest float32 squared distance -- formed as knn_reference._top forms it,
    (dx * dx + dy * dy) + dz * dz, nothing fused -- if that distance, widened, is STRICTLY below max_corr * max_corr
    (a double product); -1 / 0 otherwise.  Among target points at equal float distance the LOWEST CALLER INDEX wins:
    libwave_amd/csrc/wm_nn.hip carries a candidate as the 64-bit key (bits of d2) << 32 | index and keeps the minimum,
    and so does this function.  Non-finite points are neither queries (their row is -1 / 0) nor candidates."""
    src, tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
    q_all = transform_f(T0f, src)
    rows = np.nonzero(np.isfinite(src).all(1) & np.isfinite(q_all).all(1))[0]
    cand = np.nonzero(np.isfinite(tgt).all(1))[0]
    c = tgt[cand]
    idx = np.full(len(src), -1, np.int32)
    d2 = np.zeros(len(src), F32)
    if len(cand) == 0:
        return idx, d2
    for s in range(0, len(rows), chunk):
        r = rows[s:s + chunk]
        q = q_all[r]
        dx = q[:, None, 0] - c[None, :, 0]
        dy = q[:, None, 1] - c[None, :, 1]
        dz = q[:, None, 2] - c[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        key = ((d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand[None, :].astype(np.uint64)).min(1)
        best = (key >> np.uint64(32)).astype(np.uint32).view(F32)
        ok = best.astype(np.float64) < float(max_corr) * float(max_corr)
        idx[r[ok]] = (key[ok] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        d2[r[ok]] = best[ok]
    return idx, d2


# ------------------------------------------------------------------------------------- the Mahalanobis matrices
def mahalanobis(C1, C2, R):
    """[m, 3, 3] np.longdouble: (C2_j + R C1_i R^T)^-1 for m pairs of covariances, by the adjugate"""
    R = np.asarray(R).astype(LD)
    S = np.asarray(C2).astype(LD) + np.einsum("ab,nbc,dc->nad", R, np.asarray(C1).astype(LD), R)
    adj = np.empty_like(S)
    for a in range(3):
        for b in range(3):  # adj[a, b] = cofactor of S[b, a]
            r0, r1 = [k for k in range(3) if k != b]
            c0, c1 = [k for k in range(3) if k != a]
            minor = S[:, r0, c0] * S[:, r1, c1] - S[:, r0, c1] * S[:, r1, c0]
            adj[:, a, b] = minor if (a + b) % 2 == 0 else -minor
    det = (S[:, 0, :] * adj[:, :, 0]).sum(1)
    return adj / det[:, None, None]


def mahal_of_pairs(C1, C2, idx, T0f):
    """[n, 3, 3] float64, addressed by source index as the oracle's test hooks read it (zero rows where idx is -1):
    mahalanobis of every pair under the rotation block of T0f, rounded once"""
    M = np.zeros((len(idx), 3, 3))
    si = np.nonzero(idx >= 0)[0]
    if len(si):
        M[si] = mahalanobis(C1[si], C2[idx[si]], np.asarray(T0f, F32)[:3, :3].astype(np.float64)).astype(np.float64)
    return M


# ----------------------------------------------------------------------------------------------- the objectives
def _finish(r, Mr, p, x, m):
    """f, g[6] from the residuals r, the products Mr and the source points p (all [m, 3] longdouble)"""
    f = (r * Mr).sum() / m
    g = np.zeros(6, LD)
    g[:3] = 2 * Mr.sum(0) / m
    acc = 2 * np.einsum("nj,ni->ji", p, Mr) / m  # sum p (M r)^T
    _, dR = rotation(x)
    for a in range(3):
        g[3 + a] = (dR[a] * acc.T).sum()  # d f / d angle = (2 / m) sum (M r)^T dR p
    return float(f), g.astype(np.float64)


def fdf_pcl(src, tgt, si, ti, M, x):
    """(f, g[6]): f = (1 / m) sum r^T M r with r = T(x) p - q -- p pushed through the float matrix of x, the float
    subtraction, then widened -- and PCL's gradient of it: 2 / m sum M r (M as it is: PCL takes it for symmetric) and,
    for the angles, the trace of dR^T against 2 / m sum p (M r)^T.  M: [n_src, 3, 3], addressed by source index."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    p = src[si]
    r = (transform_f(matrix_f(x), p) - tgt[ti]).astype(LD)
    Mr = np.einsum("nab,nb->na", np.asarray(M)[si].astype(LD), r)
    return _finish(r, Mr, p.astype(LD), x, len(si))


def fdf_statistics(src, tgt, si, ti, M, T0f, x, float_matrix=True):
    """(f, g[6]) of the objective that csrc/wm_gicp_quad.hpp expands: r = r0 + (T(x) - T0) z per pair, r0 PCL's float
    residual under the pairing matrix T0f, z = (p, 1) exact, M's symmetric part.  float_matrix=False: T(x) is the exact
    (long double) matrix of x instead of PCL's float one -- a smooth function of x with the same analytic gradient,
    for finite differences."""
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    T0 = np.asarray(T0f, F32)
    p = src[si]
    r0 = (transform_f(T0, p) - tgt[ti]).astype(LD)
    if float_matrix:
        W = matrix_f(x)[:3].astype(LD)
    else:
        W = np.c_[rotation(x)[0], np.asarray(x[:3]).astype(LD)]
    D = W - T0[:3].astype(LD)
    pl = p.astype(LD)
    r = r0 + pl @ D[:, :3].T + D[:, 3]
    Ml = np.asarray(M)[si].astype(LD)
    Ms = (Ml + Ml.transpose(0, 2, 1)) / 2
    return _finish(r, np.einsum("nab,nb->na", Ms, r), pl, x, len(si))


# --------------------------------------------------------------------------------------------------- the cases
def rigid_about_centroid(cloud, t=MOTION_T, w=MOTION_W):
    """-> (moved float32 [n, 3], R, t_total): R (p - c) + c + t in float64, rounded once; c: the finite points' centroid"""
    c64 = np.asarray(cloud, np.float64)
    with np.errstate(invalid="ignore"):
        cen = c64[np.isfinite(c64).all(1)].mean(0)
        w = np.asarray(w, float)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * (K @ K)
        moved = ((c64 - cen) @ R.T + cen + np.asarray(t, float)).astype(F32)
    moved[~np.isfinite(c64).all(1)] = c64[~np.isfinite(c64).all(1)].astype(F32)  # a hole stays the hole it was
    return moved, R, cen - R @ cen + np.asarray(t, float)


class Case:
    """src, tgt: float32 [n, 3]; max_corr; x0: the pairing state, T0f = matrix_f(x0) the float matrix the pairs are found
    under; states: where the objective is evaluated -- x0, x0 + a centimetre, that + 1e-4 rad per axis; far: the cloud lies
    tens of kilometres from the origin, where x0 is the motion's own state (anything else leaves no pair within 5 m)"""

    def __init__(self, name, src, tgt, max_corr=MAX_CORR, x0=PAIR_X, far=False):
        self.name, self.far, self.max_corr = name, far, float(max_corr)
        self.src, self.tgt = np.ascontiguousarray(src, F32), np.ascontiguousarray(tgt, F32)
        self.x0 = np.asarray(x0, np.float64)
        self.T0f = matrix_f(self.x0)
        x1 = self.x0 + np.r_[STEP_T, 0, 0, 0]
        self.states = [self.x0, x1, x1 + np.r_[0, 0, 0, STEP_R]]
        self.src.setflags(write=False)
        self.tgt.setflags(write=False)
        assert len(self.src) <= 3375 and len(self.tgt) <= 3375
        self._pairs = None

    def pairs(self):
        if self._pairs is None:
            self._pairs = pairs(self.src, self.tgt, self.T0f, self.max_corr)
        return self._pairs

    def finite(self):
        """(source, target) without their non-finite rows: what the oracle's registration is given"""
        return self.src[np.isfinite(self.src).all(1)], self.tgt[np.isfinite(self.tgt).all(1)]


def group_of(case, state):
    """which entry of REF_VS_ORACLE_* the state-th state of a case falls under, for objective "statistics"; "pcl_sums"
    knows "near" and "far" only"""
    return ("far" if case.far else "near") + ("_rotated" if state == 2 else "")


def ref_vs_oracle(objective, case, state):
    g = group_of(case, state)
    if objective == "pcl_sums":
        g = g.replace("_rotated", "")
    return REF_VS_ORACLE_F[objective][g], REF_VS_ORACLE_G[objective][g]


def _far_state(R, t_total):
    """the state of a rigid motion, angles and translation rounded to float: R = Rz(psi) Ry(theta) Rx(phi)"""
    x = np.r_[t_total, math.atan2(R[2, 1], R[2, 2]), math.asin(-R[2, 0]), math.atan2(R[1, 0], R[0, 0])]
    return x.astype(F32).astype(np.float64)


def half_max_corr(src, tgt, T0f):
    """a max_corr whose double square IS the float d2, under T0f, of a source point of about median distance: about half
    the source is unmatched, and one point sits exactly on the gate (not strictly below it: not a pair)"""
    _, d2 = pairs(src, tgt, T0f, 1e3)
    for v in np.sort(d2)[len(d2) // 2:]:
        s = math.sqrt(float(v))
        if s * s == float(v):
            return s
    raise AssertionError("no float d2 is the square of a double")


def _build_cases():
    S = KR.shapes()
    out = {}
    for name in KR.NAMES:
        tgt, R, t_total = rigid_about_centroid(S[name])
        far = name.startswith("utm")
        out[name] = Case(name, S[name], tgt, x0=_far_state(R, t_total) if far else PAIR_X, far=far)
    scene = S["scene"]
    moved = out["scene"].tgt
    out["half"] = Case("half", scene, moved, max_corr=half_max_corr(scene, moved, matrix_f(PAIR_X)))
    # ... and the same with the gate taken under the IDENTITY, where a registration (one pair or batched) makes its first
    # search: there half the source is unmatched and one point sits on the gate
    out["half_start"] = Case("half_start", scene, moved, max_corr=half_max_corr(scene, moved, np.eye(4, dtype=F32)))
    # all but k source points moved 1 km away (they keep their neighbourhoods -- and covariances -- among themselves)
    for name, keep in (("no_pair", []), ("one_pair", [1234]), ("three_pairs", [7, 1234, 2900]), ("four_pairs", [7, 700, 1234, 2900])):
        src = scene.copy()
        away = np.ones(len(src), bool)
        away[keep] = False
        src[away, 0] += F32(FAR_AWAY)
        out[name] = Case(name, src, moved)
    # non-finite rows on both sides: the source's are knn_reference's `holes`, the target's partly the same rows
    tgt = moved.copy()
    tgt[3] = np.nan
    tgt[17, 0] = np.inf
    tgt[2000, 2] = -np.inf
    tgt[-1, 1] = np.nan
    out["holes_both"] = Case("holes_both", S["holes"], tgt)
    # source sizes around the 64-lane wave and the 256-thread workgroup, against the whole target
    for n in SIZES:
        out["n%d" % n] = Case("n%d" % n, scene[:n], moved)
    return out


_CASES = None
NAMES = list(KR.NAMES) + ["half", "half_start", "no_pair", "one_pair", "three_pairs", "four_pairs", "holes_both"] + ["n%d" % n for n in SIZES]


def cases():
    """name -> Case (built once)"""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
        assert list(_CASES) == NAMES
    return _CASES


def shapes():
    return cases()


def case(name):
    return cases()[name]
