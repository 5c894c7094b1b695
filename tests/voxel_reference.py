"""pcl::VoxelGrid<PointXYZ>::applyFilter (PCL 1.8, filters/impl/voxel_grid.hpp) restated in plain numpy: the checker of
voxel_downsample_dev (libwave_amd/csrc/wm_voxel.hip) and its batched twin (k_vb_*, wm_batch.hip), in the manner of
knn_reference.py / plane_reference.py.

  voxel_grid   a point counts only if its three coordinates are finite; float32 wherever PCL uses float: inv = 1 / leaf,
               min_b = (int) floorf(min * inv), ijk = (int) (floorf(p * inv) - (float) min_b) per axis; the leaf index
               ijk0 + ijk1 * dx + ijk2 * dx * dy is PCL's `unsigned int`: formed in int64 and reduced mod 2^32; a stable
               sort by (index, point number); one float32 centroid per leaf -- a sequential float32 sum in ascending
               point number (np.cumsum), then one float32 divide --, leaves in ascending index.  PCL's size rule looks
               at the TRUNCATED extents, (int64) ((max - min) * inv) + 1 per axis: if their product exceeds INT_MAX the
               input comes back as it is.  No finite point: no output.
  lattice      the numbers behind that: truncated extents, the rule, cells per axis (floor(max * inv) - floor(min * inv)
               + 1, which can be one more than the truncated extent), finite points.
  shapes       the stress clouds, seeded: name -> (cloud, leaf).  tests/test_voxel_reference_cpu.py holds voxel_grid to
               the C oracle on every one of them and the generators to their claims; tests/test_voxel_stress_gpu.py
               holds the device to voxel_grid."""
import numpy as np

INT_MAX = 2 ** 31 - 1
F = np.float32

# the device's two centroid kernels: a lane per leaf up to this many points per leaf on average, a wave per leaf beyond
WAVE_AVG = 24
LADDER = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1000]
LADDER_PAD = 100


def lattice(pts, leaf):
    """-> dict(n_valid, extents [3] (truncated, PCL's rule), rule (their product), fires, min_b [3], div_b [3] (cells per
    axis), cells (their product)); None for a cloud without a finite point"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    fin = np.isfinite(pts).all(1)
    if not fin.any():
        return None
    inv = F(1.0) / F(leaf)
    lo, hi = pts[fin].min(0), pts[fin].max(0)
    assert lo.dtype == F and ((hi - lo) * inv).dtype == F
    ext = [int(F((hi[d] - lo[d]) * inv)) + 1 for d in range(3)]
    rule = ext[0] * ext[1] * ext[2]
    min_b = [int(np.floor(F(lo[d] * inv))) for d in range(3)]
    div_b = [int(np.floor(F(hi[d] * inv))) - min_b[d] + 1 for d in range(3)]
    return dict(n_valid=int(fin.sum()), extents=ext, rule=rule, fires=rule > INT_MAX, min_b=min_b, div_b=div_b,
                cells=div_b[0] * div_b[1] * div_b[2], inv=inv, finite=fin)


def keys(pts, leaf):
    """-> (leaf index mod 2^32 of every finite point [int64], the finite points' numbers)"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    L = lattice(pts, leaf)
    rows = np.nonzero(L["finite"])[0]
    q = pts[rows]
    m = 1 << 32
    mul = [1, L["div_b"][0] % m, (L["div_b"][0] * L["div_b"][1]) % m]
    key = np.zeros(len(q), np.int64)
    for d in range(3):
        f = np.floor(q[:, d] * L["inv"]) - F(L["min_b"][d])  # float32 throughout, as PCL's static_cast<int>(floor(..) - min_b)
        assert f.dtype == F
        ijk = f.astype(np.int64)
        assert (ijk >= 0).all() and (ijk < L["div_b"][d]).all()
        key = (key + (ijk * mul[d]) % m) % m  # every product below 2^63
    return key, rows


def voxel_grid(pts, leaf):
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    L = lattice(pts, leaf)
    if L is None:
        return np.zeros((0, 3), F)
    if L["fires"]:
        return pts.copy()
    key, rows = keys(pts, leaf)
    order = np.argsort(key, kind="stable")  # stable: equal keys keep ascending point number
    ks, q = key[order], pts[rows[order]]
    heads = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    ends = np.r_[heads[1:], len(ks)]
    out = q[heads].copy()  # leaves of one point: (0 + p) / 1 = p
    for s in np.nonzero(ends - heads > 1)[0]:
        i, j = heads[s], ends[s]
        out[s] = np.cumsum(q[i:j], axis=0, dtype=F)[-1] / F(j - i)
    assert out.dtype == F
    return out


def leaf_counts(pts, leaf):
    """points per leaf, leaves in output order"""
    key, _ = keys(pts, leaf)
    return np.unique(key, return_counts=True)[1]


# ---------------------------------------------------------------------------------------------------------- the shapes
def _cells_cloud(rng, cells, counts, leaf, origin=(0, 0, 0)):
    """counts[k] points uniform inside cell cells[k] (integer ijk) of a lattice of pitch `leaf`, shuffled"""
    P = []
    for c, k in zip(cells, counts):
        u = rng.uniform(0.02, 0.98, (k, 3))  # (well inside the cell: no rounding of (c + u) * leaf crosses a boundary)
        P.append(((np.asarray(c, np.float64) - origin + u) * leaf).astype(F))
    P = np.concatenate(P)
    return P[rng.permutation(len(P))]


def ladder(pad):
    """one leaf of every size in LADDER (+ `pad` leaves of one point), scattered over an 11 x 7 x 5 lattice with a negative
    minimum, leaf 0.8"""
    rng = np.random.default_rng(11 + pad)
    counts = LADDER + [1] * pad
    pick = rng.permutation(11 * 7 * 5)[:len(counts)]
    cells = [(c % 11, (c // 11) % 7, c // 77) for c in pick]
    return _cells_cloud(rng, cells, counts, 0.8, origin=(5, 3, 2))


def threshold(extra):
    """50 leaves of exactly WAVE_AVG points and three non-finite rows (n_valid = 24 * leaves, n is not); extra = 1: one
    more point in the first leaf"""
    rng = np.random.default_rng(24)
    cells = [(i % 10, i // 10, 0) for i in range(50)]
    P = _cells_cloud(rng, cells, [WAVE_AVG] * 50, 1.0, origin=(3, 2, 0))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)
    P = np.r_[P[:500], bad[:1], P[500:900], bad[1:], P[900:]]
    if extra:
        P = np.r_[P, F([[-2.5, -1.5, 0.5]])]  # cell (0, 0, 0) of the lattice above
    return np.ascontiguousarray(P, F)


def many_leaves():
    """10 500 leaves x 25 points = 262 500 points: more leaves than the wave kernel launches waves (8 192), more than 24
    points per leaf, more points than the default radix_min (262 144)"""
    rng = np.random.default_rng(10500)
    cells = [(i % 30, (i // 30) % 25, i // 750) for i in range(10500)]
    u = rng.uniform(0.02, 0.98, (10500, 25, 3))
    P = ((np.asarray(cells, np.float64)[:, None, :] - (7, 11, 3) + u) * 1.0).astype(F).reshape(-1, 3)
    return P[rng.permutation(len(P))]


def boundaries(leaf):
    """points exactly on k * leaf, k = -40 .. 40, and one float on either side"""
    rng = np.random.default_rng(40)
    g = np.arange(-40, 41, dtype=F) * F(leaf)
    P = np.stack(np.meshgrid(g, g[::8], g[::16], indexing="ij"), -1).reshape(-1, 3)
    P = np.r_[P, np.nextafter(P, F(-np.inf)), np.nextafter(P, F(np.inf))]
    return np.ascontiguousarray(P[rng.permutation(len(P))], F)


def far(off):
    rng = np.random.default_rng(20000)
    cloud = rng.uniform(-10, 10, (20000, 3)).astype(F)
    return cloud + F([off, -off, off / 2])


def _bad_rows():
    return np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F)


def cube_1291():
    """1291^3 = 2 151 685 171 cells, truncated extents 1290^3: PCL's rule passes with a lattice in [2^31, 2^32)"""
    c = np.array([[x, y, z] for x in (-0.5, 600.2, 1289.4) for y in (-0.5, 700.3, 1289.4) for z in (-0.5, 640.1, 1289.4)], F)
    c = np.r_[c[:13], _bad_rows(), c[13:], c[5:9] + F(0.01)]  # (the last four share leaves with earlier points)
    return np.ascontiguousarray(c, F)


def cube_past_the_rule():
    """the same, x and y stretched by 1291 / 1290: the rule fires (1291 * 1291 * 1290 > INT_MAX), the cloud comes back"""
    c = cube_1291()
    c[:, :2] *= F(1291 / 1290.0)
    return c


def flat():
    """46 341 x 46 341 x 2 = 4 294 976 562 cells under a cloud thinner than a leaf that straddles z = 0: truncated extents
    46 340 x 46 340 x 1 pass the rule; 100 points twice (leaves of two), one NaN row"""
    rng = np.random.default_rng(46341)
    n = 3000
    p = np.empty((n, 3), F)
    p[:, :2] = rng.uniform(0.5, 46340.4, (n, 2))
    p[:, 2] = rng.uniform(-0.4, 0.4, n)
    p[0] = [0.5, 0.5, -0.3]
    p[1] = [46340.4, 46340.4, 0.3]
    p[100:200] = p[200:300]
    p[50] = np.nan
    return p


def column():
    """2 x 2 x 1.2e9 cells = 4 800 000 004 (truncated 1 x 1 x 1.2e9)"""
    c = np.array([[x, y, z] for x in (-0.25, 0.25) for y in (-0.25, 0.25) for z in (0.0, 3.0e8, 9.0e8, 1.2e9)], F)
    return np.ascontiguousarray(np.r_[c[:7], _bad_rows(), c[7:], c[3:9]], F)


def holes(axis):
    """400 points, every seventh non-finite (NaN, +inf, -inf in turn) in coordinate `axis` only"""
    rng = np.random.default_rng(70 + axis)
    c = rng.uniform(-4, 4, (400, 3)).astype(F)
    c[::7, axis] = np.resize(F([np.nan, np.inf, -np.inf]), len(c[::7]))
    return c


def one_finite():
    c = np.full((9, 3), np.nan, F)
    c[1, 1], c[2, 2], c[3, 0] = 1.0, np.inf, -np.inf
    c[5] = [1.25, -2.5, 1000.125]
    return c


LEAF_SIZES = {  # name -> (generator, leaf)
    "ladder_wave": (lambda: ladder(0), 0.8),            # 2 299 points in 21 leaves
    "ladder_lane": (lambda: ladder(LADDER_PAD), 0.8),   # 2 399 points in 121 leaves
    "threshold_at": (lambda: threshold(0), 1.0),
    "threshold_past": (lambda: threshold(1), 1.0),
    "many_leaves": (many_leaves, 1.0),
    "one_leaf": (lambda: np.repeat(F([[0.1, -7.3, 1e3 / 3]]), 5000, 0), 0.5),
    "boundaries_0.25": (lambda: boundaries(0.25), 0.25),
    "boundaries_0.1": (lambda: boundaries(0.1), 0.1),
    "boundaries_0.05": (lambda: boundaries(0.05), 0.05),
    "far_1e5": (lambda: far(1e5), 0.05),
    "far_3e6": (lambda: far(3e6), 0.05),
    "cube_1291": (cube_1291, 1.0),
    "cube_past_the_rule": (cube_past_the_rule, 1.0),
    "flat": (flat, 1.0),
    "column": (column, 1.0),
    "holes_x": (lambda: holes(0), 0.5),
    "holes_y": (lambda: holes(1), 0.5),
    "holes_z": (lambda: holes(2), 0.5),
    "all_non_finite": (lambda: np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3] * 3, F), 1.0),
    "one_finite": (one_finite, 1.0),
}
NAMES = list(LEAF_SIZES)
SMALL = [n for n in NAMES if n != "many_leaves"]
WIDE = ["flat", "column"]  # lattices of 2^32 cells and more that pass PCL's rule

_MADE = {}


def shape(name):
    """-> (cloud, leaf, voxel_grid(cloud, leaf)): made once, read-only"""
    if name not in _MADE:
        make, leaf = LEAF_SIZES[name]
        cloud = np.ascontiguousarray(make(), F)
        want = voxel_grid(cloud, leaf)
        cloud.setflags(write=False)
        want.setflags(write=False)
        _MADE[name] = (cloud, leaf, want)
    return _MADE[name]


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
