"""A plain numpy statement of what one ICP iteration computes AFTER its search -- the pairs PCL keeps, the 17 sums of
csrc/wm_pair_terms.hpp (icp_pair_terms), and the Umeyama / Gauss-Newton step -- and the stress cases every kernel that
forms those sums is held to, in the manner of gicp_reference.py, whose shapes and Case machinery this file reuses.

  pairs    the 1-NN of the float-transformed source in the target by brute force (gicp_reference.pairs without a gate),
           then PCL ICP's gate: a pair is REJECTED when d2 > max_corr^2 (oracle/icp.c), so a pair exactly on the gate is
           KEPT -- `half` and `half_start` have one pair more here than under GICP's strict gate
  sums     the 17 terms of a matched pair formed in float64 as icp_pair_terms forms them (products of two floats are
           exact; the GN6 terms round once per operation, nothing fused), added with math.fsum -- the correctly rounded
           sum -- together with sum |term| per component, what a summation's error bound scales with
  expand   the 17 compact sums in the public 32-slot layout (expand_stats of csrc/wm_icp_step.hpp)
  step     SVD: sigma from CENTRED points in np.longdouble, numpy's SVD, Umeyama's sign rule;  GN6: the normal equations
           in np.longdouble, numpy.linalg.lstsq -- the minimum-norm step, defined on singular systems
  disp     the largest distance between Ta p and Tb p over a set of points: the metric for two steps or two poses.  It is
           defined where a pose difference is not: on a line the rotation about the line is free, on `point` all of R
           is, and neither moves a point

Nothing of the library is imported here: tests/test_icp_reference_cpu.py holds this file to the C oracle (oracle/icp.c)
and the library's host solve to this file, tests/test_icp_stress_gpu.py holds the kernels to both."""
import math

import numpy as np

import gicp_reference as GR

LD = np.longdouble
F32 = np.float32
SVD, GN6 = 0, 1  # wm_icp_params::mode
MODES = (("svd", SVD), ("gn6", GN6))

PAIRS_K = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)  # matched pairs around the wave, kBlock and kSmThreads
EXTRA_SIZES = (1023, 1024)  # beside gicp_reference's n1025
AWAY = 100.0  # the unmatched rows of a pairsK source: 100 m above a scene that is 8 m high
# step(GN6): singular values of the centred J^T J below this fraction of the largest count as zero.  The points are
# float32: a direction that only their own rounding constrains (a line whose points are collinear up to 2^-24 of their
# coordinates) has an eigenvalue of 2^-48 = 3.6e-15 of the largest, and lstsq's default (1.3e-15) would solve for it.
# 1e-12 is the level at which the library calls a system singular (kGnPivotTol, csrc/wm_math.hpp).
RCOND = 1e-12
# the cases whose minimiser is a family of poses (collinear or coincident pairs)
FREE = {"line", "line_x", "line_diag", "line_far", "point", "collinear3"}

# disp (metres) between the reference's own two forms on each case's pairs, (SVD, GN6): wm.umeyama_from_stats /
# wm.gn6_from_stats on the correctly rounded sums of sums() -- the library's formula -- against step(), over
# compare_points(); the larger of the two poses the GPU tests pair under (the case's own and the identity).  None: the library refuses the system (GN6
# on the FREE cases: J^T J is singular, WM_CONV_DEGENERATE).  Recomputed and held by tests/test_icp_reference_cpu.py
# (it fails if a value here is below the recomputed one or more than ten times above it); the measured value rounded
# up to its second digit, 1e-16 where it is below that.
#   SVD near the origin: last bits.  utm / utm_plane: Sqp / n - qm pm^T cancels seven to eight digits 55 km out.
#   line_diag, line_far (SVD): the float32 points are collinear only up to their own rounding (2e-6 m at 20 m); the
#   rotation about the line is decided by that noise, differently in each form, and moves such a point by up to its
#   distance from the line.
REF_FORMS = {
    "exact_plane": (4.3e-15, 1.0e-16), "noisy_plane": (8.2e-15, 1.0e-16), "line": (4.5e-15, None),
    "point": (1.0e-16, None), "clumps_outliers": (2.3e-13, 3.9e-14), "shell": (5.3e-15, 1.0e-16),
    "lattice": (8.3e-15, 1.0e-16), "dups": (2.2e-14, 1.0e-16), "utm": (1.2e-08, 4.1e-10),
    "utm_plane": (2.6e-09, 3.0e-09), "scene": (2.7e-14, 8.0e-16), "holes": (5.0e-14, 1.6e-15),
    "half": (2.0e-14, 2.5e-16), "half_start": (3.1e-14, 8.2e-16), "three_pairs": (9.2e-13, 5.7e-15),
    "four_pairs": (3.6e-13, 1.5e-15), "holes_both": (2.6e-14, 1.6e-15), "n10": (2.0e-14, 6.0e-16),
    "n63": (2.1e-14, 1.2e-15), "n64": (2.3e-14, 1.0e-16), "n65": (3.9e-14, 7.2e-16), "n255": (8.6e-15, 1.6e-15),
    "n256": (3.0e-14, 2.2e-16), "n257": (3.8e-14, 1.3e-15), "n513": (2.3e-14, 9.1e-16), "n1025": (1.8e-14, 1.1e-15),
    "n1023": (4.6e-14, 1.4e-15), "n1024": (2.0e-14, 1.7e-16), "line_x": (2.4e-15, None),
    "line_diag": (5.5e-07, None), "line_far": (1.5e-07, None), "mirror": (1.4e-14, 1.3e-14),
    "mirror_thin": (5.3e-15, 1.0e-16), "collinear3": (3.2e-13, None), "mm": (1.0e-16, 1.0e-16),
    "pairs63": (1.7e-14, 8.5e-16), "pairs64": (8.4e-14, 1.3e-16), "pairs65": (4.3e-14, 7.0e-16),
    "pairs255": (5.4e-14, 1.2e-15), "pairs256": (2.5e-14, 2.3e-16), "pairs257": (5.5e-14, 9.5e-16),
    "pairs1023": (9.6e-14, 5.5e-16), "pairs1024": (4.7e-14, 2.0e-16), "pairs1025": (6.4e-14, 1.1e-15),
}


# ------------------------------------------------------------------------------------------------- the pairs
def pairs(src, tgt, Tf, max_corr):
    """-> (idx [n] int32, d2 [n] float32): every source point's nearest target point under the float matrix Tf, as
    gicp_reference.pairs finds it (float32 distances, ties to the lowest index, non-finite rows neither queries nor
    candidates), kept when (double) d2 <= max_corr * max_corr -- PCL ICP's gate; -1 / 0 otherwise."""
    idx, d2 = GR.pairs(src, tgt, Tf, 1e18)  # (no gate: every float32 distance is below 1e36)
    drop = (idx < 0) | (d2.astype(np.float64) > float(max_corr) * float(max_corr))
    idx = np.where(drop, -1, idx).astype(np.int32)
    return idx, np.where(drop, F32(0), d2).astype(F32)


def matched(src, tgt, Tf, idx):
    """-> (rows, p, q): the matched source rows, those points under Tf (float32) and their matches (float32)"""
    si = np.nonzero(idx >= 0)[0]
    return si, GR.transform_f(Tf, np.asarray(src, F32)[si]), np.asarray(tgt, F32)[idx[si]]


# -------------------------------------------------------------------------------------------------- the sums
def terms(p, q, d2, mode):
    """[m, 17] float64: icp_pair_terms of every pair -- n, p | SVD: t, t p^T row by row | GN6: A^T A's upper triangle of
    the rotation block, r = p - t, p x r | d2"""
    p, q = np.asarray(p, F32).astype(np.float64), np.asarray(q, F32).astype(np.float64)
    px, py, pz = p.T
    tx, ty, tz = q.T
    one = np.ones(len(p))
    if mode == SVD:
        cols = [one, px, py, pz, tx, ty, tz, tx * px, tx * py, tx * pz, ty * px, ty * py, ty * pz, tz * px, tz * py, tz * pz]
    else:
        rx, ry, rz = px - tx, py - ty, pz - tz
        cols = [one, px, py, pz, py * py + pz * pz, -px * py, -px * pz, px * px + pz * pz, -py * pz, px * px + py * py,
                rx, ry, rz, py * rz - pz * ry, pz * rx - px * rz, px * ry - py * rx]
    cols.append(np.asarray(d2, F32).astype(np.float64))
    return np.stack(cols, 1) if len(p) else np.zeros((0, 17))


def expand(a, mode):
    """the 17 compact sums -> the public 32 slots, as expand_stats lays them out (slots 29-31 carry counters: left 0)"""
    st = np.zeros(32)
    if mode == SVD:
        st[:17] = a
        return st
    n, sx, sy, sz = a[:4]
    H = np.zeros((6, 6))
    H[0, 0] = H[1, 1] = H[2, 2] = n
    H[0, 4], H[0, 5], H[1, 3], H[1, 5], H[2, 3], H[2, 4] = sz, -sy, -sz, sx, sy, -sx
    H[3, 3], H[3, 4], H[3, 5], H[4, 4], H[4, 5], H[5, 5] = a[4:10]
    st[0], st[1] = n, a[16]
    st[2:23] = H[np.triu_indices(6)]
    st[23:29] = a[10:16]
    return st


def sums(p, q, d2, mode):
    """-> (st [32], scale [32]) in the public layout: the correctly rounded sums of terms(), and sum |term| of the same
    components (the scale of slot k is that of the compact sum it copies, whatever its sign)"""
    t = terms(p, q, d2, mode)
    a = np.array([math.fsum(t[:, k]) for k in range(17)])
    s = np.array([math.fsum(np.abs(t[:, k])) for k in range(17)])
    return expand(a, mode), np.abs(expand(s, mode))


# -------------------------------------------------------------------------------------------------- the step
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    a, b = (1.0, 0.5) if th < 1e-12 else (math.sin(th) / th, (1.0 - math.cos(th)) / (th * th))
    return np.eye(3) + a * K + b * (K @ K)


def step(p, q, mode):
    """-> T [4, 4] float64 of one step from the pairs (p, q).
    SVD: pcl::umeyama without scaling -- sigma = (1 / n) sum (q - qm)(p - pm)^T from the centred points in long double,
    rounded once; R = U diag(1, 1, s) V^T with s = -1 iff det(U) det(V) < 0; t = qm - R pm in long double.
    GN6: (J^T J) delta = -J^T r with J = [I | -[p]x], r = p - q, summed in long double; delta = the minimum-norm
    least-squares solution; T = [exp(dw) | dt].  The equations are formed about the pairs' centroid c --
    r + dt + dw x p = r + (dt + dw x c) + dw x (p - c): the same step wherever J^T J is regular, from a 6 x 6 whose
    condition does not grow with the fourth power of the distance from the origin (1e17 for `utm` otherwise: beyond
    what lstsq can tell from singular) -- and dt = dt' - dw x c in long double."""
    pl, ql = np.asarray(p, F32).astype(LD), np.asarray(q, F32).astype(LD)
    n = len(pl)
    T = np.eye(4)
    if mode == SVD:
        pm, qm = pl.sum(0) / LD(n), ql.sum(0) / LD(n)
        sigma = ((ql - qm).T @ (pl - pm) / LD(n)).astype(np.float64)
        U, _, Vt = np.linalg.svd(sigma)
        s = -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0
        R = U @ np.diag([1.0, 1.0, s]) @ Vt
        T[:3, :3] = R
        T[:3, 3] = (qm - R.astype(LD) @ pm).astype(np.float64)
        return T
    r = pl - ql
    c = pl.sum(0) / LD(n)
    pc = pl - c
    J = np.zeros((n, 3, 6), LD)
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1
    J[:, 0, 4], J[:, 0, 5] = pc[:, 2], -pc[:, 1]
    J[:, 1, 3], J[:, 1, 5] = -pc[:, 2], pc[:, 0]
    J[:, 2, 3], J[:, 2, 4] = pc[:, 1], -pc[:, 0]
    H = np.einsum("nca,ncb->ab", J, J).astype(np.float64)
    g = np.einsum("nca,nc->a", J, r).astype(np.float64)
    delta = np.linalg.lstsq(H, -g, rcond=RCOND)[0]
    dw = delta[3:].astype(LD)
    T[:3, :3] = rodrigues(delta[3:])
    T[:3, 3] = (delta[:3].astype(LD) - np.cross(dw, c)).astype(np.float64)
    return T


def disp(Ta, Tb, pts):
    """the largest |Ta p - Tb p| over pts, in float64 (formed from the DIFFERENCE of the two poses: 55 km out the two
    images agree in their first eleven digits)"""
    P = np.asarray(pts, np.float64)
    if len(P) == 0:
        return 0.0
    D = np.asarray(Ta, np.float64)[:3] - np.asarray(Tb, np.float64)[:3]
    return float(np.linalg.norm(P @ D[:, :3].T + D[:, 3], axis=1).max())


def ssr(T, p, q):
    """sum |T p - q|^2 in long double (a float64 pose, float32 points)"""
    Tl = np.asarray(T, np.float64).astype(LD)
    r = np.asarray(p, F32).astype(LD) @ Tl[:3, :3].T + Tl[:3, 3] - np.asarray(q, F32).astype(LD)
    return float((r * r).sum())


def rigid_error(T):
    """(|R R^T - I| max, |det R - 1|) of a pose"""
    R = np.asarray(T, np.float64)[:3, :3]
    return float(np.abs(R @ R.T - np.eye(3)).max()), float(abs(np.linalg.det(R) - 1.0))


def ssr_slack(delta, T_ref, p, q):
    """by how much sum |T p - q|^2 can exceed sum |T_ref p - q|^2 when T moves no point further than delta from where
    T_ref does: |r + e|^2 - |r|^2 <= 2 |r| |e| + |e|^2 per pair, e <= delta"""
    Tl = np.asarray(T_ref, np.float64).astype(LD)
    r = np.asarray(p, F32).astype(LD) @ Tl[:3, :3].T + Tl[:3, 3] - np.asarray(q, F32).astype(LD)
    return float(2.0 * delta * np.sqrt((r * r).sum(1)).sum() + len(r) * delta * delta)


def pose_floor(p, q):
    """what a float64 pose cannot resolve at these coordinates: a few ulps of the largest coordinate (the last bit of
    t, and of R's entries times |p|)"""
    big = max(float(np.abs(np.asarray(p, np.float64)).max()), float(np.abs(np.asarray(q, np.float64)).max()), 1e-300)
    return 8.0 * np.spacing(big)


# --------------------------------------------------------------------------------------------------- the cases
class Case(GR.Case):
    """a gicp_reference.Case under ICP's pairing: pairs() keeps the pair on the gate; pairs_at(Tf) is the same search
    under another float matrix (the identity: where a registration makes its first search), kept per matrix"""

    def __init__(self, name, src, tgt, max_corr=GR.MAX_CORR, x0=GR.PAIR_X, far=False):
        super().__init__(name, src, tgt, max_corr=max_corr, x0=x0, far=far)
        self._at = {}

    def pairs_at(self, Tf):
        Tf = np.ascontiguousarray(Tf, F32)
        key = Tf.tobytes()
        if key not in self._at:
            self._at[key] = pairs(self.src, self.tgt, Tf, self.max_corr)
        return self._at[key]

    def pairs(self):
        return self.pairs_at(self.T0f)

    def pairs_identity(self):
        return self.pairs_at(np.eye(4, dtype=F32))


def _line(rng, n, direction, offset):
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    return (rng.uniform(-20, 20, n)[:, None] * d + np.asarray(offset, np.float64)).astype(F32)


def _spread(n, k):
    """k of n rows, spread evenly through the order"""
    return np.unique(np.floor(np.arange(k) * (n / float(k))).astype(np.int64))


def _build_cases():
    G = GR.cases()
    out = {}
    for name in GR.NAMES:
        g = G[name]
        out[name] = Case(name, g.src, g.tgt, max_corr=g.max_corr, x0=g.x0, far=g.far)
    scene, moved = G["scene"].src, G["scene"].tgt
    for n in EXTRA_SIZES:
        out["n%d" % n] = Case("n%d" % n, scene[:n], moved)
    # collinear sources against collinear targets: along an axis THROUGH the origin (y = z = 0: the GN6 terms -px * pz
    # and -py * pz are -0.0), along (1, 1, 1) / sqrt 3, and along a random direction 20 m off the origin
    rng = np.random.default_rng(201)
    u = rng.normal(size=3)
    off = rng.normal(size=3)
    off = 20.0 * off / np.linalg.norm(off)
    for name, direction, offset in (("line_x", (1, 0, 0), (0, 0, 0)), ("line_diag", (1, 1, 1), (0, 0, 0)), ("line_far", u, off)):
        src = _line(rng, 1000, direction, offset)
        out[name] = Case(name, src, GR.rigid_about_centroid(src)[0])
    # the target mirrored in z about its centroid: a rigid answer (det +1) must come back
    mir = moved.astype(np.float64)
    mir[:, 2] = 2.0 * mir[:, 2].mean() - mir[:, 2]
    out["mirror"] = Case("mirror", scene, mir.astype(F32))
    # ... which nearest-neighbour pairing defeats on a cloud 8 m high with points a metre apart: a point pairs with
    # whatever of the mirrored target is NEAR it, so sigma keeps a positive determinant (tests/test_icp_reference_cpu.py
    # asserts which case reaches the branch).  A slab thinner than its points' spacing pairs every point with its own
    # image: noisy_plane (1 cm thick, points 36 cm apart), sigma's third direction is -var(z), det(U) det(V) < 0.
    thin = G["noisy_plane"]
    mir = thin.tgt.astype(np.float64)
    mir[:, 2] = 2.0 * mir[:, 2].mean() - mir[:, 2]
    out["mirror_thin"] = Case("mirror_thin", thin.src, mir.astype(F32))
    # exactly three matched pairs, collinear (sigma has rank 1; n >= 3 passes PCL's test), the rest 1 km away
    src = scene.copy()
    src[:, 0] += F32(GR.FAR_AWAY)
    a = moved[1234].astype(np.float64)
    d = np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])
    for row, s in ((7, -1.0), (1234, 0.25), (2900, 1.5)):
        src[row] = (a + s * d).astype(F32)
    out["collinear3"] = Case("collinear3", src, moved)
    # coordinates of centimetres: the bins hold trunc(x * 2^56), and a product of two such coordinates is below 2^-12
    mm = (scene.astype(np.float64) * 1e-3).astype(F32)
    x0 = np.r_[np.asarray(GR.PAIR_X[:3]) * 1e-3, GR.PAIR_X[3:]]
    out["mm"] = Case("mm", mm, GR.rigid_about_centroid(mm, t=tuple(1e-3 * v for v in GR.MOTION_T))[0], max_corr=GR.MAX_CORR * 1e-3, x0=x0)
    # exactly K contributing rows of 3 000, spread through the source's order; four non-finite rows among them; the others
    # AWAY above the scene (8 m high) -- unmatched lanes inside waves whose other lanes contribute
    for k in PAIRS_K:
        rows = _spread(len(scene), k + 4)
        assert len(rows) == k + 4
        holes = rows[[len(rows) // 5, 2 * len(rows) // 5, 3 * len(rows) // 5, 4 * len(rows) // 5]]
        src = scene.copy()
        away = np.ones(len(src), bool)
        away[rows] = False
        src[away, 2] += F32(AWAY)
        src[holes[0]] = np.nan
        src[holes[1], 1] = np.inf
        src[holes[2], 2] = -np.inf
        src[holes[3], 0] = np.nan
        out["pairs%d" % k] = Case("pairs%d" % k, src, moved)
    return out


NEW = ["n%d" % n for n in EXTRA_SIZES] + ["line_x", "line_diag", "line_far", "mirror", "mirror_thin", "collinear3", "mm"] + ["pairs%d" % k for k in PAIRS_K]
NAMES = list(GR.NAMES) + NEW
_CASES = None


def cases():
    """name -> Case (built once)"""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
        assert list(_CASES) == NAMES
    return _CASES


def case(name):
    return cases()[name]


def finite_src(c):
    return c.src[np.isfinite(c.src).all(1)]


def _extent(c):
    pts = np.r_[finite_src(c), c.tgt[np.isfinite(c.tgt).all(1)]].astype(np.float64)
    return np.abs(pts).max(0)


def float_pose_floor(c):
    """A WORST-CASE ESTIMATE, not a bound derived from the iteration -- held by experiment:
    tests/test_icp_reference_cpu.py::test_far_registrations_scatter_by_the_float_pose runs icp_loop (below) on the far
    cases with the pose turned by 1e-9 rad after the first step and finds its results up to 3.9e-3 m apart, inside this
    figure and far outside helpers.TOL_T.
    How far two registrations of SEVERAL iterations may end apart (disp) because the pose a search runs under is
    PCL's float matrix: an entry of R near 1 rounds by up to 2^-25, which moves coordinate i of a point by up to
    2^-25 (|x| + |y| + |z|), and the transformed coordinate rounds by half an ulp of itself.  Each registration settles
    on the minimiser of ITS rounded cloud; a last-bit difference of the double pose flips such a rounding, for every
    point alike.  Twice (two registrations) the vector of those per-coordinate bounds: 3e-5 m for a cloud 50 m from the
    origin -- where it is not needed, the paths take the same roundings and agree to 1e-9 m -- and 1.4e-2 m at 55 km,
    where the float32 points themselves are 4 mm apart.  Used for the `far` cases only."""
    ext = _extent(c)
    per = 2.0 ** -25 * ext.sum() + 0.5 * np.spacing(ext.astype(F32)).astype(np.float64)
    return float(2.0 * np.linalg.norm(per))


def line_floor(c):
    """how far two equally good registrations of a FREE case may end apart over its matched points: the float32 points
    (and their float transforms) lie within sqrt(3) half-ulps of their line, twice over; a rotation about the line -- free
    -- moves a point by at most twice its distance from the line"""
    return float(2.0 * np.sqrt(3.0) * np.spacing(F32(_extent(c).max())))


def icp_loop(c, nn, P=None, force=0, max_iter=30, fit_eps=1e-2, t_eps=1e-8):
    """pcl::IterativeClosestPoint as oracle/icp.c states it (incremental_float = 0), with step(SVD) as its estimator: the
    double pose rounded to float for every search, PCL's gate, DefaultConvergenceCriteria.  nn(points) -> (idx, d2) over
    the case's finite target.  P: a 4 x 4 applied to the pose after the FIRST step -- the experiment's perturbation.
    -> (T, iterations, state, idx of the last search, its mean squared distance)"""
    src, tgt = c.finite()
    T, prev, it = np.eye(4), np.inf, 0
    while True:
        moved = GR.transform_f(T.astype(F32), src)
        oi, od = nn(moved)
        keep = od.astype(np.float64) <= c.max_corr * c.max_corr
        idx = np.where(keep, oi, -1)
        mse = math.fsum(od[keep].astype(np.float64)) / int(keep.sum())
        Tk = step(moved[keep], tgt[oi[keep]], SVD)
        T = Tk @ T
        if P is not None and it == 0:
            T = P @ T
        it += 1
        if force:
            if it >= force:
                return T, it, "FORCED", idx, mse
            continue
        if it >= max_iter:
            return T, it, "ITERATIONS", idx, mse
        if 0.5 * (np.trace(Tk[:3, :3]) - 1.0) >= 1.0 - t_eps and float((Tk[:3, 3] ** 2).sum()) <= t_eps:
            return T, it, "TRANSFORM", idx, mse
        if abs(mse - prev) < 1e-12:
            return T, it, "ABS_MSE", idx, mse
        if np.isfinite(prev) and abs(mse - prev) / prev < fit_eps:
            return T, it, "REL_MSE", idx, mse
        prev = mse


def compare_points(c, Tf, p):
    """the points two steps of a case are compared over (disp): the finite source points under the pairing matrix Tf --
    unmatched ones included, a kilometre from the pairs in `three_pairs` -- except on the FREE cases, where only the
    matched points p are: a rotation about the pairs' line is free there and moves everything off the line"""
    return p if c.name in FREE else GR.transform_f(Tf, finite_src(c))
