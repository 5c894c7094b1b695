"""wm_cluster_extract_cond (libwave_amd/csrc/wm_cluster.hip) restated in float32 numpy + scipy: the checker of
tests/test_cluster_cond_gpu.py, built on cluster_reference.py (its edges of the distance test, its _finish).

  edges     two different finite points i, j are joined iff d2 < r2 (cluster_reference's strict float32 test) AND
            with a normal angle:  |dot| >= cos_min, dot = (a0_i * a0_j + a1_i * a1_j) + a2_i * a2_j as float32 arrays
                                  (every operation rounded, none fused), cos_min = float32(math.cos(angle));
            with a scalar diff:   |s_i - s_j| <= float32(max_scalar_diff), the subtraction one float32 operation.
            A NaN makes its comparison false (numpy's comparisons, as the device's).  angle / diff None: test off.
  the rest  cluster_reference._finish: components, the size rule, the order, the labels.
  two forms components_brute: every pair of finite points goes through the distance test, in chunks, and every pair
            that passes through the attribute tests.  components: the candidate pairs of a float64 kd-tree, the
            float32 tests re-formed on them.  tests/test_cluster_cond_reference_cpu.py holds the two to each other.

The shapes of the table of hand-checked component counts (corner, fan, pair, triple) are
built here, read-only and once."""
import math

import numpy as np

import cluster_reference as CR

NONE, REJECTED, INT_MAX = CR.NONE, CR.REJECTED, CR.INT_MAX


def cos_min(angle):
    return np.float32(math.cos(float(angle)))


def edge_ok(attr, a, b, angle=None, diff=None):
    """The attribute tests on the pairs (a[k], b[k]) of rows of attr (float32 [n, >= 4]) -> a bool per pair."""
    attr = np.asarray(attr, np.float32)
    ok = np.ones(len(a), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if angle is not None:
            p, q = attr[a], attr[b]
            dot = (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]
            assert dot.dtype == np.float32
            ok &= np.abs(dot) >= cos_min(angle)
        if diff is not None:
            d = attr[a, 3] - attr[b, 3]
            assert d.dtype == np.float32
            ok &= np.abs(d) <= np.float32(diff)
    return ok


def _brute_edges(cloud, tolerance, chunk=256):
    """cluster_reference.components_brute's pairs: -> (cand, rows, cols), positions in cand, each pair once."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    cand = np.nonzero(np.isfinite(cloud).all(1))[0]
    c = cloud[cand]
    r2 = CR._r2(tolerance)
    rows, cols = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for s in range(0, len(cand), chunk):
        q = c[s:s + chunk]
        dx = q[:, None, 0] - c[None, :, 0]
        dy = q[:, None, 1] - c[None, :, 1]
        dz = q[:, None, 2] - c[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        upper = np.arange(len(cand))[None, :] > np.arange(s, s + len(q))[:, None]
        a, b = np.nonzero((d2 < r2) & upper)
        rows.append(a + s)
        cols.append(b)
    return cand, np.concatenate(rows), np.concatenate(cols)


def _kd_edges(cloud, tolerance):
    """cluster_reference.components' pairs: a float64 kd-tree's candidates, the float32 distance test on them."""
    from scipy.spatial import cKDTree
    cloud = np.ascontiguousarray(cloud, np.float32)
    cand = np.nonzero(np.isfinite(cloud).all(1))[0]
    c = cloud[cand]
    rows = cols = np.zeros(0, np.int64)
    if len(cand) > 1:
        pairs = cKDTree(c.astype(np.float64)).query_pairs(float(tolerance) * 1.001 + 1e-6, output_type="ndarray")
        a, b = c[pairs[:, 0]], c[pairs[:, 1]]
        dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        ok = d2 < CR._r2(tolerance)
        rows, cols = pairs[ok, 0].astype(np.int64), pairs[ok, 1].astype(np.int64)
    return cand, rows, cols


def _restrict(n, edges, attr, angle, diff, min_cluster_size, max_cluster_size):
    cand, rows, cols = edges
    ok = edge_ok(attr, cand[rows], cand[cols], angle, diff)
    return CR._finish(n, cand, rows[ok], cols[ok], min_cluster_size, max_cluster_size, dict(n_near=len(rows)))


def components_brute(cloud, attr, tolerance, angle=None, diff=None, min_cluster_size=1, max_cluster_size=INT_MAX):
    """Every pair of finite points.  n_near: the pairs that pass the distance test; n_edges: ... and the others."""
    return _restrict(len(cloud), _brute_edges(cloud, tolerance), attr, angle, diff, min_cluster_size, max_cluster_size)


def components(cloud, attr, tolerance, angle=None, diff=None, min_cluster_size=1, max_cluster_size=INT_MAX):
    """Candidate pairs from a float64 kd-tree, the float32 tests on them."""
    return _restrict(len(cloud), _kd_edges(cloud, tolerance), attr, angle, diff, min_cluster_size, max_cluster_size)


# ------------------------------------------------------------------ cluster_reference.CASES under conditions
DEG = math.pi / 180.0
NORMAL_K = 10
# (angle, diff): normal 10 deg, normal 45 deg, scalar on the curvature at 0.01, both flags together
CONDITIONS = [(10 * DEG, None), (45 * DEG, None), (None, 0.01), (10 * DEG, 0.01)]
BIG_TOLERANCE, BIG_ANGLE = 0.1, 30 * DEG

_EDGES = {}


def case_edges(name, tolerance):
    """The all-pairs distance edges of a named shape of cluster_reference, computed once for all conditions."""
    key = (name, float(tolerance))
    if key not in _EDGES:
        _EDGES[key] = _brute_edges(CR.shapes()[name], tolerance)
    return _EDGES[key]


def brute_case(name, tolerance, attr, angle, diff):
    """components_brute of a named shape with the default size rule (the distance pass shared between conditions)."""
    return _restrict(len(CR.shapes()[name]), case_edges(name, tolerance), attr, angle, diff, 1, INT_MAX)


def pca_attributes(cloud, k=NORMAL_K):
    """(nx, ny, nz, curvature) of the k nearest neighbours' covariance in float64 numpy, rounded to float32; zeros for a
    non-finite point.  What stands in for wm_estimate_normals where there is no device: the two forms of the checker
    must agree whatever the attributes are, and these have the statistics of the device's."""
    from scipy.spatial import cKDTree
    cloud = np.ascontiguousarray(cloud, np.float32)
    out = np.zeros((len(cloud), 4), np.float32)
    cand = np.nonzero(np.isfinite(cloud).all(1))[0]
    c = cloud[cand].astype(np.float64)
    k = min(k, len(cand))
    if k < 3:
        return out
    nb = c[cKDTree(c).query(c, k)[1]]
    d = nb - nb.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d) / k)
    tr = w.sum(1)
    out[cand, :3] = v[:, :, 0]
    out[cand, 3] = np.where(tr > 0, w[:, 0] / np.where(tr > 0, tr, 1.0), 0.0)
    return out


# ------------------------------------------------------------------ the shapes of the table
def _build_shapes():
    rng = np.random.default_rng(413)
    g = np.arange(32, dtype=np.float64) * 0.1
    u, v = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    z = np.zeros_like(u)
    floor = np.c_[u, v, z]                    # z = 0
    wall = np.c_[z, u, v + 0.1]               # x = 0, z = 0.1 ... 3.2
    cloud = np.r_[floor, wall].astype(np.float32)
    attr = np.zeros((2048, 4), np.float32)
    attr[:1024, 2] = 1.0
    attr[1024:, 0] = 1.0
    perm = rng.permutation(2048)
    corner = (np.ascontiguousarray(cloud[perm]), np.ascontiguousarray(attr[perm]))

    i = np.arange(64)
    fan_cloud = np.c_[i * 0.125, np.zeros(64), np.zeros(64)].astype(np.float32)  # exactly representable
    ang = i * 5.0 * DEG
    fan_attr = np.c_[np.cos(ang), np.sin(ang), np.zeros(64), 0.5 * i].astype(np.float32)
    out = dict(corner=corner, fan=(fan_cloud, fan_attr))
    for pair in out.values():
        for a in pair:
            a.setflags(write=False)
    return out


_SHAPES = None


def shapes():
    """name -> (cloud float32 [n, 3], attr float32 [n, 4]), read-only, built once."""
    global _SHAPES
    if _SHAPES is None:
        _SHAPES = _build_shapes()
    return _SHAPES


def pair(c):
    """Two points 0.125 m apart, normals (1, 0, 0) and (c, sqrt(1 - c^2), 0): their dot is exactly c."""
    c = np.float32(c)
    cloud = np.float32([[0, 0, 0], [0.125, 0, 0]])
    attr = np.float32([[1, 0, 0, 0], [c, np.sqrt(np.float32(1) - c * c), 0, 0]])
    return cloud, attr


def triple(middle_s=1.0, middle_normal=(0.0, 0.0, 1.0)):
    """Three mutually close points, s = 0, middle_s, 2, normals (0, 0, 1) but the middle one's."""
    cloud = np.float32([[0, 0, 0], [0.05, 0, 0], [0.1, 0, 0]])
    attr = np.float32([[0, 0, 1, 0], list(middle_normal) + [middle_s], [0, 0, 1, 2]])
    return cloud, attr


# the table of hand-checked counts: (what, cloud, attr, tolerance, angle, diff) -> the components and the sizes of the largest
def table():
    corner, fan = shapes()["corner"], shapes()["fan"]
    half = np.float32(0.5)
    below = np.nextafter(np.float32(0.75), np.float32(0))
    acos75 = math.acos(0.75)
    assert cos_min(acos75) == np.float32(0.75)
    t3 = triple()
    t2 = (np.ascontiguousarray(t3[0][[0, 2]]), np.ascontiguousarray(t3[1][[0, 2]]))
    return [
        ("corner no test", corner, 0.15, None, None, 1, [2048]),
        ("corner normal 30", corner, 0.15, 30 * DEG, None, 2, [1024, 1024]),
        ("corner normal pi/2", corner, 0.15, math.pi / 2, None, 2, [1024, 1024]),
        ("fan 0.2 normal 30", fan, 0.2, 30 * DEG, None, 1, [64]),
        ("fan 0.2 normal 4", fan, 0.2, 4 * DEG, None, 64, [1]),
        ("fan 0.3 normal 7.5", fan, 0.3, 7.5 * DEG, None, 1, [64]),
        ("fan 0.2 scalar 0.5", fan, 0.2, None, 0.5, 1, [64]),
        ("fan 0.3 scalar 0.5", fan, 0.3, None, 0.5, 1, [64]),
        ("fan 0.2 scalar below 0.5", fan, 0.2, None, float(np.nextafter(half, np.float32(0))), 64, [1]),
        ("fan 0.3 scalar below 0.5", fan, 0.3, None, float(np.nextafter(half, np.float32(0))), 64, [1]),
        ("pair c = 0.75", pair(0.75), 0.25, acos75, None, 1, [2]),
        ("pair c below 0.75", pair(below), 0.25, acos75, None, 2, [1, 1]),
        ("triple scalar 1", t3, 0.2, None, 1.0, 1, [3]),
        ("triple without the middle", t2, 0.2, None, 1.0, 2, [1, 1]),
        ("triple middle s NaN", triple(middle_s=np.nan), 0.2, None, 5.0, 2, [2, 1]),
        ("triple middle normal zero", triple(middle_normal=(0.0, 0.0, 0.0)), 0.2, 30 * DEG, None, 2, [2, 1]),
    ]


def big_case(attr):
    """components of cluster_reference's large scene at BIG_TOLERANCE with the normal test at BIG_ANGLE."""
    return components(CR.big_cloud(), attr, BIG_TOLERANCE, BIG_ANGLE, None)
