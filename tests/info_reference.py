"""An independent float64 restatement of libwave's three post-match information estimators
(ICPMatcher::estimateCensi, wave_matching/src/icp.cpp:167-397; estimateLUM / estimateLUMold,
wave_matching/src/icp_pcl_functions.cpp:51-289), written from the calculus of their costs.  It shares
no code with oracle/ (the literal C restatement of the reference's text) nor with the HIP kernels
(libwave_amd/csrc/wm_info.hip), so that the two can be checked against something neither was made from.

Censi.  With x = (t, theta), z = (a, b) for one pair (a = the matched TARGET point, the reference's
Z1..Z3; b = the SOURCE point, Z4..Z6) and J(x) = sum_i |R(theta) a_i + t - b_i|^2, the estimate is
info = (H^-1 M H^-1)^-1 with H = d2J/dx2 and M = sum_i D_i cov_Z,i D_i^T.  Three conventions of the
reference are kept as they are (the contract is parity; none of them is "fixed" here):

  (a) parametrisation -- R(theta) = Rz(theta2) Ry(theta1) Rx(theta0), the expanded expressions of
      icp.cpp:262-312 (d2J_dX2) and :322-368 (d2J_dZdX) are exactly the derivatives of that cost; but
      theta is `result.rotation().eulerAngles(0, 1, 2)` (icp.cpp:175), Eigen's decomposition of the
      rotation as Rx Ry Rz.  Away from identity R(theta) is therefore NOT the result's rotation, and the
      Hessian of the Rx Ry Rz cost differs from the reference's by O(1) in the coupling entries.
  (b) mixed term -- D_i = d2J_i/dz dx is stored with rows = z and columns = x (icp.cpp:208-211, 322-368)
      and accumulated as middle += D cov_Z D^T (icp.cpp:370), not the textbook D^T cov_Z D.
  (c) spherical Jacobian -- cov_Z = j diag(lin, ang, ang, lin, ang, ang) j^T with j as the reference
      writes it (icp.cpp:225-246): range, bearing and azimuth from the float coordinates in float
      (std::sqrt / std::atan2 / std::atan of float arguments), az = atan(z / sqrt(x^2 + y^2)) an
      elevation plugged into formulas written for a polar angle.  (0, 0, 0) gives atan(0 / 0) = NaN;
      a point on the z axis atan(+-inf) = +-pi / 2.

LUM / LUMold.  tests/golden/make_golden.py's lum_info (already independent of the oracle and the
kernels) is used as it is; `lum` below adds only the choice of how s^2 is summed (the reference's
sequential float sum, or the exact sum of the same float terms) and scipy's exact search for LUMold.
"""
import math
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import lum_info, lum_normal_equations  # noqa: E402


# ------------------------------------------------------------------ rotations
def elem(axis, angle, order=0):
    """Rotation about `axis` (0 x, 1 y, 2 z) by `angle`, or its `order`-th derivative in the angle."""
    c, s = math.cos(angle), math.sin(angle)
    cc, ss = [(c, s), (-s, c), (-c, -s)][order]   # (cos, sin) differentiated `order` times
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.zeros((3, 3))
    if order == 0:
        R[axis, axis] = 1.0
    R[i, i] = R[j, j] = cc
    R[i, j] = -ss
    R[j, i] = ss
    return R


def rotation_and_derivatives(theta, order=(2, 1, 0)):
    """R = E_order[0] E_order[1] E_order[2] (default Rz Ry Rx: convention (a)) at theta = (about x, about y,
    about z); dR[k] = dR/dtheta_k and d2R[k][l] = d2R/dtheta_k dtheta_l."""
    def comp(d):
        out = np.eye(3)
        for ax in order:
            out = out @ elem(ax, theta[ax], d[ax])
        return out
    unit = np.eye(3, dtype=int)
    R = comp((0, 0, 0))
    dR = [comp(unit[k]) for k in range(3)]
    d2R = [[comp(unit[k] + unit[l]) for l in range(3)] for k in range(3)]
    return R, dR, d2R


def euler_012(R):
    """Eigen 3.3 MatrixBase::eulerAngles(0, 1, 2): R = Rx(e0) Ry(e1) Rz(e2) with e0 in [0, pi].  The
    decomposition is computed for the inverse rotation and negated; when that first angle comes out
    positive it is moved by -pi and the second is taken on the other side (c2 -> -c2): the flip
    branch, whose results lie near (pi + roll, pi - pitch, yaw +- pi)."""
    r0 = math.atan2(R[1, 2], R[2, 2])
    c2 = math.sqrt(R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1])
    if r0 > 0.0:
        r0 -= math.pi
        r1 = math.atan2(-R[0, 2], -c2)
    else:
        r1 = math.atan2(-R[0, 2], c2)
    s1, c1 = math.sin(r0), math.cos(r0)
    r2 = math.atan2(s1 * R[2, 0] - c1 * R[1, 0], c1 * R[1, 1] - s1 * R[2, 1])
    return np.array([-r0, -r1, -r2])


def euler_flipped(R):
    """True when euler_012(R) takes Eigen's flip branch (the inverse rotation's first angle > 0)."""
    return math.atan2(R[1, 2], R[2, 2]) > 0.0


# ------------------------------------------------------------------ Censi
def spherical_jacobian(xyz, sd):
    """Convention (c): d(point)/d(range, bearing, azimuth) with the three scalars formed in float, the
    columns scaled by the standard deviations sd (3,).  Returns (n, 3, 3) float64."""
    p = np.asarray(xyz, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    f = lambda v: v.astype(np.float32).astype(np.float64)   # round to float (numpy's float32 atan is not)
    with np.errstate(invalid="ignore", divide="ignore"):
        rg = f(np.sqrt((x * x + y * y) + z * z))
        br = f(np.arctan2(y.astype(np.float64), x.astype(np.float64)))
        az = f(np.arctan((z / np.sqrt(x * x + y * y)).astype(np.float64)))
        cb, sb, ca, sa = np.cos(br), np.sin(br), np.cos(az), np.sin(az)
        J = np.zeros((len(p), 3, 3))
        J[:, 0, 0], J[:, 1, 0], J[:, 2, 0] = cb * sa, sb * sa, ca
        J[:, 0, 1], J[:, 1, 1] = -rg * sb * sa, rg * cb * sa
        J[:, 0, 2], J[:, 1, 2], J[:, 2, 2] = rg * cb * ca, rg * ca * sb, -rg * sa
    return J * np.asarray(sd, np.float64)[None, None, :]


def censi(ref_pts, tgt_pts, T, lin_covar=2.5e-4, ang_covar=7.78e-9, order=(2, 1, 0), chunk=1 << 16):
    """estimateCensi on explicit pairs (ref_pts[i] = b_i, the source point; tgt_pts[i] = a_i, its match)
    at the result T.  Returns dict(info, H, M, theta).  `order` is for the convention check only."""
    b_all = np.asarray(ref_pts, np.float32).astype(np.float64)
    a_all = np.asarray(tgt_pts, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    theta = euler_012(T[:3, :3])
    R, dR, d2R = rotation_and_derivatives(theta, order)
    t = T[:3, 3]
    sd = np.sqrt([lin_covar, ang_covar, ang_covar])
    H = np.zeros((6, 6))
    M = np.zeros((6, 6))
    n = len(a_all)
    H[:3, :3] = 2.0 * n * np.eye(3)
    for lo in range(0, n, chunk):
        a, b = a_all[lo:lo + chunk], b_all[lo:lo + chunk]
        e = a @ R.T + t - b                                  # residual of each pair
        Ra = [a @ dR[k].T for k in range(3)]                 # de/dtheta_k
        # d2J/dx2 of |e|^2: 2 (de/dx_k . de/dx_l + e . d2e/dx_k dx_l)
        for k in range(3):
            H[:3, 3 + k] += 2.0 * Ra[k].sum(0)
            for l in range(3):
                H[3 + k, 3 + l] += 2.0 * np.einsum("ij,ij->", Ra[k], Ra[l]) + \
                    2.0 * np.einsum("ij,ij->", e, a @ d2R[k][l].T)
        # D = d2J/dz dx, rows z = (a, b), columns x = (t, theta)          -- convention (b)
        D = np.zeros((len(a), 6, 6))
        D[:, :3, :3] = 2.0 * R.T                             # d/da (2 e)
        D[:, 3:, :3] = -2.0 * np.eye(3)                      # d/db (2 e)
        for k in range(3):
            D[:, :3, 3 + k] = 2.0 * (Ra[k] @ R + e @ dR[k])  # d/da (2 e . R_k a) = 2 (R^T R_k a + R_k^T e)
            D[:, 3:, 3 + k] = -2.0 * Ra[k]                   # d/db (2 e . R_k a)
        K = np.zeros((len(a), 6, 6))                         # cov_Z = K K^T, block diagonal  -- convention (c)
        K[:, :3, :3] = spherical_jacobian(tgt_pts[lo:lo + chunk], sd)
        K[:, 3:, 3:] = spherical_jacobian(ref_pts[lo:lo + chunk], sd)
        DK = np.einsum("nij,njk->nik", D, K)
        M += np.einsum("nik,njk->ij", DK, DK)
    H[3:, :3] = H[:3, 3:].T
    # (H^-1 M H^-1)^-1 = H M^-1 H: the same matrix without inverting a product whose condition is cond(H)^2 cond(M)
    if not np.isfinite(M).all():   # a NaN Jacobian (a point at the origin) poisons every entry
        return dict(info=np.full((6, 6), np.nan), H=H, M=M, theta=theta)
    info = H @ np.linalg.solve(M, H)
    return dict(info=info, H=H, M=M, theta=theta)


def info_tolerance(H, M, rel=1e-7):
    """Bound on max |info - info'| when H and M carry errors of `rel` times their largest entry (the
    reference's float sub-products: 2 * Z3 * Z4 and the like are rounded to float) and info' is formed
    literally as (H^-1 M H^-1)^-1 in double.  The first-order perturbation of info = H M^-1 H in 2-norms,
    |dH| |M^-1 H| + |H M^-1| |dH| + |H M^-1| |dM| |M^-1 H|, plus the literal form's own rounding,
    ~u cond(H)^2 cond(M) |info| (u = 2^-53): both carry the measured conditions of H and M."""
    dH = rel * np.abs(H).max() * 6.0
    dM = rel * np.abs(M).max() * 6.0
    A = np.linalg.norm(H @ np.linalg.inv(M), 2)
    info = H @ np.linalg.solve(M, H)
    literal = 64 * 2.0 ** -53 * np.linalg.cond(H) ** 2 * np.linalg.cond(M) * np.linalg.norm(info, 2)
    return 2.0 * dH * A + dM * A * A + literal


# ------------------------------------------------------------------ LUM / LUMold
def lum(final, tgt, pairs=None, max_corr=None, exact_ss=False):
    """estimateLUM (pairs = (i, j): the align's own correspondences) or estimateLUMold (pairs None: scipy's
    exact nearest neighbour with the strict gate d2 < max_corr^2).  exact_ss: s^2 as the exact sum of the
    reference's float terms (math.fsum) instead of its sequential float sum.  Returns dict(info, MM, ss, n)."""
    i, j = lumold_pairs(final, tgt, max_corr) if pairs is None else pairs
    MM, _, terms = lum_normal_equations(final[i], tgt[j])
    if not exact_ss:
        info, n, ss = lum_info(final, tgt, pairs=(i, j))
        return dict(info=info, MM=MM, ss=ss, n=n)
    ss = float(np.float32(math.fsum(terms.astype(np.float64))))
    return dict(info=MM * float(np.float32(1.0) / np.float32(ss)), MM=MM, ss=ss, n=len(i))


def lumold_pairs(final, tgt, max_corr):
    """estimateLUMold's own search (icp_pcl_functions.cpp:67-101): exact NN, kept when d2 < max_corr^2."""
    _, j = cKDTree(tgt.astype(np.float64)).query(final.astype(np.float64))
    diff = final - tgt[j]
    d2 = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    keep = d2.astype(np.float64) < max_corr * max_corr
    return np.flatnonzero(keep), j[keep]
