"""A plain numpy statement of what the NDT kernels compute, and the stress shapes they are held to.

model(): pcl::VoxelGridCovariance<PointXYZ>::applyFilter as NDTMatcher uses it -- membership by the float product
floor(p * (1 / res)), at least 6 points, the covariance scaled by (n - 1) / n, eigenvalues below a hundredth of the largest
raised to it -- with the covariance formed from CENTRED data (two passes) instead of PCL's raw sums, eigenvalues by
np.linalg.eigh instead of a Jacobi iteration.  score_gradient(): computeDerivatives' score and gradient over the 27 cells
around each transformed point, the rotational columns of the point Jacobian from products of the elementary rotations'
derivatives instead of PCL's table of eight vectors.  Nothing of the device side is imported: tests/test_ndt_reference_cpu.py
holds this file to the C oracle (oracle/ndt.c), tests/test_ndt_stress_gpu.py holds the kernels to both.

shapes(): where a voxel model or a 27-cell look-up can go wrong without the reference scan noticing -- see each builder."""
import math

import numpy as np

# Bounds on the difference between this file and the oracle over every shape and pose of shapes(): the worst values
# that tests/test_ndt_reference_cpu.py prints (it fails if one is exceeded), rounded up by less than a factor of two.  Two
# correct restatements in double, differing in the order of their sums, in raw sums against centred data and in the
# eigen-solver; the worst cases are the oracle's raw sums on the 5 cm voxels of `outliers64`.
#   inverse covariances, relative to the voxel's largest entry (measured: 5.34e-10 on outliers64; 5.0e-12 elsewhere)
REF_VS_ORACLE_ICOV = 1e-9
#   the score relative to itself (measured: 5.23e-12, `line` moved almost out of its target)
REF_VS_ORACLE_SCORE = 1e-11
#   the gradient relative to its largest entry -- and, on the far shapes, its translation block relative to ITS largest
#   entry (measured: 2.77e-11 on too_wide, 1.74e-11 on outliers64, 7.0e-12 elsewhere)
REF_VS_ORACLE_GRAD = 5e-11

MIN_POINTS = 6  # min_points_per_voxel_
SHIFT = (0.125, -0.25, 0.125)  # the translation `lattice`'s registration has to find; a pose of every shape
ROT_POSE = (0.05, -0.02, 0.01, 0.004, -0.003, 0.006)


def _inv_res(res):
    return np.float32(1.0) / np.float32(res)  # inverse_leaf_size_ is a float


def cells_of(pts, res):
    """(n, 3) int64 cell numbers of FINITE float32 points: the float product, as PCL"""
    return np.floor(np.asarray(pts, np.float32) * _inv_res(res)).astype(np.int64)


def lattice_dims(tgt, res):
    """cells per axis of the lattice over the finite points' bounding box"""
    t = np.asarray(tgt, np.float32)
    c = cells_of(t[np.isfinite(t).all(1)], res)
    return [int(v) for v in c.max(0) - c.min(0) + 1]


def model(tgt, res):
    """{(i, j, k): (n, mean, cov, icov, valid)} for every occupied voxel; cov / icov None where the voxel has fewer than
    6 points or PCL rejects its eigenvalues"""
    t32 = np.asarray(tgt, np.float32)
    t32 = t32[np.isfinite(t32).all(1)]
    cell = cells_of(t32, res)
    order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))  # stable: points of a voxel keep their order
    cs, P = cell[order], t32[order].astype(np.float64)
    brk = np.r_[0, np.nonzero((np.diff(cs, axis=0) != 0).any(1))[0] + 1, len(cs)] if len(cs) else [0]
    out = {}
    for a, b in zip(brk[:-1], brk[1:]):
        n, p = int(b - a), P[a:b]
        origin = np.floor(p.min(0))  # an integer near the voxel: p - origin is exact in double
        c = p - origin
        m = c.sum(0) / n
        mean = origin + m
        cov = icov = None
        valid = False
        if n >= MIN_POINTS:
            d = c - m
            cov = (d.T @ d) / n * ((n - 1.0) / n)  # PCL: pp / n - mean mean^T, then (n - 1) / n
            w, V = np.linalg.eigh(cov)
            if not (w[0] < 0 or w[1] < 0 or w[2] <= 0):
                lo = 0.01 * w[2]  # min_covar_eigvalue_mult_
                if w[0] < lo:
                    w = w.copy()
                    w[0] = lo
                    if w[1] < lo:
                        w[1] = lo
                    cov = V @ np.diag(w) @ np.linalg.inv(V)
                icov = np.linalg.inv(cov)
                valid = bool(np.isfinite(icov).all())
        out[tuple(int(v) for v in cs[a])] = (n, mean, cov, icov, valid)
    return out


def gauss_constants(res, outlier_ratio=0.55):
    c1, c2 = 10.0 * (1.0 - outlier_ratio), outlier_ratio / res ** 3
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    d2 = -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def _cs(angle, snap):
    if snap and abs(angle) < 10e-5:  # computeAngleDerivatives
        return 1.0, 0.0
    return math.cos(angle), math.sin(angle)


def _rotations(pose, snap):
    """Rx, Ry, Rz and their derivatives by their own angle (3 x 3 float64 each)"""
    (cx, sx), (cy, sy), (cz, sz) = (_cs(float(pose[k]), snap) for k in (3, 4, 5))
    R = [np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], float), np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], float),
         np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], float)]
    D = [np.array([[0, 0, 0], [0, -sx, -cx], [0, cx, -sx]], float), np.array([[-sy, 0, cy], [0, 0, 0], [-cy, 0, -sy]], float),
         np.array([[-sz, -cz, 0], [cz, -sz, 0], [0, 0, 0]], float)]
    return R, D


def pose_matrix_f(pose):
    """PCL's final_transformation_: Translation * Rx * Ry * Rz with float sines and cosines of the float angles, every
    product and sum rounded to float (a correctly rounded cosf: the double result rounded once)"""
    f = np.float32
    (cx, sx), (cy, sy), (cz, sz) = ((f(math.cos(float(f(pose[k])))), f(math.sin(float(f(pose[k]))))) for k in (3, 4, 5))
    T = np.zeros((3, 4), np.float32)
    T[0, :3] = [cy * cz, -cy * sz, sy]
    T[1, :3] = [cx * sz + sx * sy * cz, cx * cz - sx * sy * sz, -sx * cy]
    T[2, :3] = [sx * sz - cx * sy * cz, sx * cz + cx * sy * sz, cx * cy]
    T[:, 3] = [f(pose[0]), f(pose[1]), f(pose[2])]
    return T


NEIGHBOURS = [(di, dj, dk) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)]  # ascending (k, j, i)


def score_gradient(src, pose, mdl, res, outlier_ratio=0.55):
    """(score, gradient[6]) of computeDerivatives at `pose` for the FINITE rows of src over the valid voxels of mdl"""
    d1, d2 = gauss_constants(res, outlier_ratio)
    s32 = np.asarray(src, np.float32)
    s32 = s32[np.isfinite(s32).all(1)]
    if len(s32) == 0:
        return 0.0, np.zeros(6)
    T = pose_matrix_f(pose)
    xt = np.stack([((T[r, 0] * s32[:, 0] + T[r, 1] * s32[:, 1]) + T[r, 2] * s32[:, 2]) + T[r, 3] for r in range(3)], 1)
    assert xt.dtype == np.float32
    cell = np.floor(xt * _inv_res(res)).astype(np.int64)
    keys = [k for k, v in mdl.items() if v[4]]
    slot = {k: n for n, k in enumerate(keys)}
    mean = np.array([mdl[k][1] for k in keys]).reshape(-1, 3)
    icov = np.array([mdl[k][3] for k in keys]).reshape(-1, 3, 3)
    mean_f = mean.astype(np.float32)  # the kd-tree of centroids is a float one
    # the point Jacobian's rotational columns: d(Rx Ry Rz)/d(angle) x
    R, D = _rotations(pose, snap=True)
    x = s32.astype(np.float64)
    Jrot = [x @ (D[0] @ R[1] @ R[2]).T, x @ (R[0] @ D[1] @ R[2]).T, x @ (R[0] @ R[1] @ D[2]).T]
    score_terms, grad_terms = [], []
    for di, dj, dk in NEIGHBOURS:
        idx = np.array([slot.get((int(c[0]) + di, int(c[1]) + dj, int(c[2]) + dk), -1) for c in cell])
        pt = np.nonzero(idx >= 0)[0]
        if len(pt) == 0:
            continue
        v = idx[pt]
        f = xt[pt] - mean_f[v]
        dd = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]
        assert dd.dtype == np.float32
        near = dd.astype(np.float64) < res * res
        pt, v = pt[near], v[near]
        xx = xt[pt].astype(np.float64) - mean[v]
        cx = np.einsum("nab,nb->na", icov[v], xx)
        q = np.einsum("na,na->n", xx, cx)
        e = np.exp(-d2 * q / 2.0)
        w = d2 * e
        ok = ~((w > 1) | (w < 0) | np.isnan(w))
        pt, cx, e, w = pt[ok], cx[ok], e[ok], w[ok] * d1
        score_terms.append(-d1 * e)
        g = np.empty((len(pt), 6))
        g[:, :3] = cx * w[:, None]
        for k in range(3):
            g[:, 3 + k] = np.einsum("na,na->n", cx, Jrot[k][pt]) * w
        grad_terms.append(g)
    if not score_terms:
        return 0.0, np.zeros(6)
    return float(np.concatenate(score_terms).sum()), np.concatenate(grad_terms).sum(0)


# --------------------------------------------------------------------------------------------------------- the shapes
class Shape:
    """tgt, src: float32 (n, 3); res; poses: where the derivatives are compared; far: |cell| reaches 2^20 (translation
    poses only: a rotation throws every point out of the lattice); extra: what single tests need besides"""

    def __init__(self, tgt, src, res, far=False, **extra):
        self.tgt = np.ascontiguousarray(tgt, np.float32)
        self.src = np.ascontiguousarray(src, np.float32)
        self.res = res
        self.far = far
        # (translations of a quarter and half a voxel, exact floats at res 0.5; one small rotation)
        self.poses = [np.zeros(6), np.array(SHIFT + (0, 0, 0), float) * (res / 0.5), np.array([-0.25, 0.125, 0, 0, 0, 0]) * (res / 0.5)]
        if not far:
            self.poses.append(np.array(ROT_POSE) * np.array([res / 0.5] * 3 + [1, 1, 1]))
        self.extra = extra
        assert len(self.tgt) <= 20000 and len(self.src) <= 3000


def _lattice_base():
    """Voxel size 0.5, every coordinate a multiple of 0.125: four positions per axis and voxel, each occupied voxel
    holding exactly 8 distinct points -- sums of such numbers are exact in double wherever the cloud lies, so a
    translation by whole voxels translates the model and nothing else.  24 x 20 x 6 voxels around the origin (negative
    cells on every axis), 60 % of them occupied."""
    rng = np.random.default_rng(5)
    cells = np.stack(np.meshgrid(np.arange(-12, 12), np.arange(-10, 10), np.arange(-3, 3), indexing="ij"), -1).reshape(-1, 3)
    cells = cells[rng.random(len(cells)) < 0.6]
    pts = []
    for c in cells:
        sel = rng.choice(64, 8, replace=False)
        pts.append(c * 0.5 + np.stack([sel % 4, (sel // 4) % 4, sel // 16], 1) * 0.125)
    base = np.concatenate(pts)
    pick = rng.choice(len(base), 3000, replace=False)
    src = base[pick[:1500]] + rng.integers(-2, 3, (1500, 3)) * 0.125  # derivatives: target points moved by eighths
    moved = base[pick] - np.array(SHIFT)  # registrations: 3 000 target points, all moved by SHIFT
    return base, src, moved


def _lattice(offset=(0.0, 0.0, 0.0)):
    base, src, moved = _lattice_base()
    D = np.array(offset, float)
    out = []
    for a in (base, src, moved):
        f = (a + D).astype(np.float32)
        assert np.array_equal(f.astype(np.float64), a + D)  # the float cast is exact: multiples of 1/8 below 2^20
        out.append(f)
    return Shape(out[0], out[1], 0.5, far=bool(D.any()), moved=out[2], offset=D)


UTM = (600000.0, -700000.0, 1000.0)
UTM_NEG = (-1000000.0, 900000.0, 0.0)
UTM_EDGE = (524288.0, -524288.0, 0.0)  # cell 2^20 on x, cell -2^20 on y: the lattice has cells on both sides of each


def _slab():
    """a plane with noise of 1e-3 res across it: the smallest eigenvalue is raised, well clear of rounding"""
    rng = np.random.default_rng(11)
    tgt = np.c_[rng.uniform(-5, 5, (8000, 2)), rng.normal(0, 5e-4, 8000)]
    src = tgt[::4] + rng.normal(0, 0.02, (2000, 3))
    return Shape(tgt, src, 0.5, moved=tgt[::4][:2000] - np.array(SHIFT) * 0.4)


def _line():
    """a line with such noise: two eigenvalues raised"""
    rng = np.random.default_rng(12)
    tgt = np.c_[rng.uniform(-20, 20, 6000), rng.normal(0, 5e-4, (6000, 2))]
    src = tgt[::3] + rng.normal(0, 0.02, (2000, 3))
    return Shape(tgt, src, 0.5)


def _plane_exact():
    """z = 0 exactly, x and y multiples of 1/8: the covariance's z row is exactly zero, the lattice one cell thick"""
    rng = np.random.default_rng(13)
    tgt = np.c_[rng.integers(-40, 40, (8000, 2)) * 0.125, np.zeros(8000)]
    src = tgt[::4] + rng.integers(-2, 3, (2000, 3)) * 0.125
    return Shape(tgt, src, 0.5)


def _threshold():
    """voxels of 5, 6 and 7 points (four each), six coincident points, and a few ordinary voxels; `tgt_none`: no voxel
    reaches 6 points"""
    rng = np.random.default_rng(14)
    pts, none = [], []
    for k, n in enumerate([5, 6, 7] * 4):
        corner = np.array([(k % 4) * 1.5 - 2.0, (k // 4) * 1.5 - 2.0, 0.0])
        pts.append(corner + rng.uniform(0.02, 0.48, (n, 3)))
        none.append(corner + rng.uniform(0.02, 0.48, (min(n, 5), 3)))
    pts.append(np.tile([4.25, 0.25, 0.25], (6, 1)))  # sums of these are exact: the covariance is exactly zero
    for k in range(6):
        pts.append(np.array([-4.0 + 0.5 * k, 3.0, 0.5]) + rng.uniform(0.02, 0.48, (20, 3)))
    tgt = np.concatenate(pts)
    src = np.concatenate([tgt + rng.normal(0, 0.1, tgt.shape) for _ in range(3)])
    return Shape(tgt, src, 0.5, tgt_none=np.concatenate(none).astype(np.float32))


def _faces(res):
    """points exactly on voxel faces -- float(k * res), which for res 0.3 the float product puts into cell k or (k = 3) into
    cell k - 1 --,
    negative coordinates and -0.0, among points inside that keep every voxel's covariance regular"""
    rng = np.random.default_rng(15)
    f = np.float32
    cells = np.stack(np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3)
    pts = []
    for c in cells:
        p = ((c + rng.uniform(0.05, 0.95, (10, 3))) * res).astype(f)
        for r in range(4):  # four of the ten: one, two or three coordinates on a face of the voxel
            on = rng.random(3) < 0.5
            on[rng.integers(3)] = True
            p[r, on] = (c[on] * res).astype(f)
        pts.append(p)
    tgt = np.concatenate(pts)
    tgt[tgt == 0] = f(-0.0)
    assert np.signbit(tgt[tgt == 0]).all() and (tgt == 0).sum() > 50
    k = rng.integers(-5, 6, (1500, 3))
    src = ((k + rng.uniform(0, 1, (1500, 3))) * res).astype(f)
    on = rng.random((1500, 3)) < 0.4
    src[on] = (k * res).astype(f)[on]
    src[::7][src[::7] == 0] = f(-0.0)
    return Shape(tgt, src, res, moved=tgt[::2][:1200] - np.array(SHIFT, f) * f(0.2))


def _crowded():
    """one voxel of 5 000 points next to voxels of 31, 32, 33 and 127, 128, 129 -- either side of both thresholds between
    a lane's walk and a wave's sums (32 for the few voxels of this grid, 128 for large grids and as an option) -- among
    enough ordinary voxels that the grid is not one where every voxel is a wave's"""
    rng = np.random.default_rng(16)
    counts = [(0, 0, 0, 5000)] + [(1 + k, 0, 0, n) for k, n in enumerate((31, 32, 33))] + \
             [(k - 1, 1, 0, n) for k, n in enumerate((127, 128, 129))]
    counts += [(i, j, k, 10) for i in range(-3, 5) for j in range(-3, 5) for k in (-1, 1)]
    tgt = np.concatenate([(np.array([i, j, k]) + rng.uniform(0.02, 0.98, (n, 3))) * 0.5 for i, j, k, n in counts])
    tgt = tgt[rng.permutation(len(tgt))]  # a voxel's points are not in a row
    assert len(tgt) <= 192 * len(counts)
    src = tgt[:2500] + rng.normal(0, 0.05, (2500, 3))
    return Shape(tgt, src, 0.5, moved=tgt[:2500] - np.array(SHIFT) * 0.2, counts=sorted(c[3] for c in counts))


def _far_clump(rng, corner):
    """8 distinct points on a 1/128 lattice inside the res-0.05 voxel above `corner` (a multiple of 1/128 that is a
    voxel's low corner): their sums are exact in double at 60 km"""
    sel = rng.choice(125, 8, replace=False)
    return np.asarray(corner, float) + (np.stack([sel % 5, (sel // 5) % 5, sel // 25], 1) + 1) / 128.0


def _outliers(wide):
    """clumps inside 10 m at res 0.05 plus two 8-point voxels 20 km out on every axis' far sides: the lattice has more than
    2^32 cells (64-bit sort keys) and no dense table (the hash grid), by the code's own rules; wide: one more at 60 km, a
    span of more than 2^20 voxels"""
    rng = np.random.default_rng(17)
    centres = rng.uniform(-5, 5, (60, 3))
    near = np.concatenate([c + rng.uniform(0, 0.1, (100, 3)) for c in centres])
    far = [_far_clump(rng, (20000.0, 20000.0, 2000.0)), _far_clump(rng, (-20000.0, -20000.0, -2000.0))]
    if wide:
        far.append(_far_clump(rng, (60000.0, 0.0, 0.0)))
    tgt = np.concatenate([near] + far)
    f = tgt.astype(np.float32)
    assert np.array_equal(f[len(near):].astype(np.float64), tgt[len(near):])
    src = np.concatenate([near[::3] + rng.normal(0, 0.01, (2000, 3))] + [c + rng.integers(-3, 4, (8, 3)) / 128.0 for c in far])
    return Shape(f, src, 0.05)


def _holes():
    """NaN, +inf and -inf rows in the target AND in the source, and finite garbage of magnitude 1e9 in the source"""
    rng = np.random.default_rng(18)
    tgt = np.r_[np.c_[rng.uniform(-6, 6, (6000, 2)), rng.normal(0, 0.02, 6000)], rng.uniform(-3, 3, (6000, 3))].astype(np.float32)
    src = (tgt[::6] + rng.normal(0, 0.05, (2000, 3))).astype(np.float32)
    for cloud, step in ((tgt, 97), (src, 41)):
        for k, bad in enumerate((np.nan, np.inf, -np.inf)):
            for axis in range(3):
                cloud[3 * k + axis + 1::step * 9, axis] = bad
    src[5::250] = rng.choice([-1e9, 1e9], (8, 3))
    src[6::250, 0] = 1e9
    return Shape(tgt, src, 0.5)


_BUILDERS = {
    "lattice": _lattice, "utm": lambda: _lattice(UTM), "utm_neg": lambda: _lattice(UTM_NEG), "utm_edge": lambda: _lattice(UTM_EDGE),
    "slab": _slab, "line": _line, "plane_exact": _plane_exact, "threshold": _threshold, "faces": lambda: _faces(0.5),
    "faces_03": lambda: _faces(0.3), "crowded": _crowded, "outliers64": lambda: _outliers(False),
    "too_wide": lambda: _outliers(True), "holes": _holes}
NAMES = list(_BUILDERS)
_cache = {}


def shape(name):
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def shapes():
    return {name: shape(name) for name in NAMES}
